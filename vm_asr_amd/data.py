"""Training and evaluation on a folder of wav files: the reference's data loader (data_loader/data_loaders.py:25-79,82-520) with
every signal-processing step on the device.

    SyntheticVCTK(config, length, sr_in, seed)               dataset of seeded noise clips with the same batch contract (no files)
    WavFolder(config, training, root=None)                   dataset: (wave (1, n) CPU, file_sr, name) per clip, nothing else
    collate_clips(samples)                                   -> (waves (B, 1, n_max) zero-padded, lengths, rates, names)
    PrepareOnDevice(loader, config, device, training, seed)  yields (wave_in, wave_tgt, highcut, name, pad) on `device`
    get_loader(config, device, logger=None)                  (train, validation) loaders, or the test loader with EVAL_MODE

Same flow as the reference: `<root>/<speaker>/<speaker>_<utt>.wav`, speakers sorted, the first DATA.TRAIN_SPLIT[0] for training and
the rest for testing, DATA.USE_QUANTITY of the shuffled training ids; a training clip is the file's first
int(DATA.SEGMENT * DATA.FLAC2WAV.SRC_SR) frames, a test clip the whole file; the clip is brought to the target rate, its tail filled
with white noise (torch.randn * DATA.PAD_WHITENOISE) up to the segment (training) or the next multiple of it (testing), and the
input is the target resampled down to a drawn rate and up again.

Built differently: the dataset (and so every DataLoader worker process) only decodes — `inferencer.read_wav`, standard library —
and never touches the GPU; the main process copies a collated batch to the device once and runs resampling to the target rate
(`resample_poly`, clips of one file rate in one call), the noise tail and the degradation (`resample.degrade_batch`: filters
designed on the device, the whole batch at per-clip rates in two launches) there.  A training clip that is longer than a segment
after resampling (a file below the target rate) is cut to the segment, so every training batch is (B, 1, segment); the reference
would pad it to a multiple and then fail to collate.  Deliberate deviations from the reference: DESIGN.md §7.
"""
import os
import random

import numpy as np
import torch

from . import resample
from .inferencer import read_wav
from .tester import frames_per_segment

__all__ = ["SyntheticVCTK", "WavFolder", "collate_clips", "PrepareOnDevice", "get_loader"]


class SyntheticVCTK(torch.utils.data.Dataset):
    """Synthetic clips with the reference's batch contract
    `(wave_in (1,T), wave_tgt (1,T), highcut int64, name, pad)` — CustomVCTK_092._load_sample
    (data_loader/data_loaders.py:490-513); T = int(SEGMENT * TARGET_SR) (:138-140);
    highcut = int((n_fft/2+1) * sr_in / sr_tgt) (:482-486).  Seeds follow SURVEY.md §8d."""

    def __init__(self, config, length=64, sr_in=16000, seed=123):
        self.T = int(config.DATA.SEGMENT * config.DATA.TARGET_SR)
        self.n = length
        self.seed = seed
        self.highcut = int((config.DATA.STFT.N_FFT // 2 + 1) * sr_in / config.DATA.TARGET_SR)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + i)
        tgt = 0.1 * torch.randn(1, self.T, generator=g)
        g2 = torch.Generator().manual_seed(self.seed + 1 + 7919 * (i + 1))
        inp = 0.1 * torch.randn(1, self.T, generator=g2)
        return inp, tgt, torch.tensor(self.highcut, dtype=torch.int64), f"synthetic_{i:06d}", 0


class WavFolder(torch.utils.data.Dataset):
    """The clips of `<root>/<speaker>/<speaker>_<utt>.wav` (root: join(DATA.DATA_PATH, DATA.FLAC2WAV.DST_PATH)) of the training or
    the test speakers.  `__getitem__` -> (wave (1, n) float32 mono on the CPU, the file's sample rate, file name)."""

    def __init__(self, config, training, root=None):
        self.config, self.training = config, bool(training)
        self.root = root or os.path.join(config.DATA.DATA_PATH, config.DATA.FLAC2WAV.DST_PATH)
        if not os.path.isdir(self.root):
            raise FileNotFoundError(f"{self.root}: no such directory (expected <speaker>/<speaker>_<utt>.wav below it)")
        if str(config.DATA.RESAMPLER) != "scipy":
            raise ValueError(f"DATA.RESAMPLER {config.DATA.RESAMPLER!r}: only scipy's polyphase resampler exists here (DESIGN.md §7)")
        self.num_frames = int(config.DATA.SEGMENT * config.DATA.FLAC2WAV.SRC_SR)
        speakers = sorted(d for d in os.listdir(self.root) if os.path.isdir(os.path.join(self.root, d)))
        split = int(config.DATA.TRAIN_SPLIT[0])
        self.speakers = speakers[:split] if self.training else speakers[split:]
        ids = [(s, f) for s in self.speakers for f in sorted(os.listdir(os.path.join(self.root, s)))
               if f.endswith(".wav") and f.startswith(s + "_")]
        if self.training:
            q = float(config.DATA.USE_QUANTITY)
            if not 0.0 < q <= 1.0:
                raise ValueError("Quantity should be between 0 and 1")
            random.Random(config.SEED).shuffle(ids)
            ids = ids[:int(len(ids) * q)]
        self.ids = ids

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, n):
        speaker, name = self.ids[n]
        audio, sr = read_wav(os.path.join(self.root, speaker, name))
        if self.training:
            audio = audio[:, :self.num_frames]
        return audio.mean(dim=0, keepdim=True), sr, name


def collate_clips(samples):
    """[(wave (1, n_i), rate_i, name_i)] -> (waves (B, 1, max n_i) zero-padded at the end, lengths [n_i], rates, names)."""
    lengths = [int(w.shape[-1]) for w, _, _ in samples]
    waves = torch.zeros(len(samples), 1, max(lengths), dtype=torch.float32)
    for i, (w, _, _) in enumerate(samples):
        waves[i, :, :lengths[i]] = w
    return waves, lengths, [int(r) for _, r, _ in samples], [n for _, _, n in samples]


def pad_length(n, seg):
    """White-noise samples the reference appends to n samples (data_loaders.py:371-389)."""
    return seg - n if n < seg else (seg - n % seg) % seg


class PrepareOnDevice:
    """Wraps a loader of `collate_clips` batches; yields the batch contract of SyntheticVCTK,
    `(wave_in (B,1,T), wave_tgt (B,1,T), highcut (B) int64, names, pad (B) int64)`, waves on `device`.  Training: T is the segment
    and the input rate of each clip is drawn (uniformly from DATA.RANDOM_RESAMPLE, or by DATA.WEIGHTED_SR as data_loaders.py:439-453)
    from random.Random(seed) / numpy.random.default_rng(seed); testing: T is the longest clip padded to a multiple of the segment
    and the rate is TAG's input rate.  The noise comes from a generator on `device` seeded with `seed`."""

    def __init__(self, loader, config, device, training, seed=0):
        self.loader, self.config, self.device, self.training = loader, config, torch.device(device), bool(training)
        self.target_sr = int(config.DATA.TARGET_SR) if self.training else int(str(config.TAG).split("_")[1])
        self.seg = frames_per_segment(config, self.target_sr)
        self.seed = seed
        self._rng, self._np_rng, self._gen = random.Random(seed), np.random.default_rng(seed), None

    def __len__(self):
        return len(self.loader)

    def draw_rate(self):
        d = self.config.DATA
        if not self.training:
            return int(str(self.config.TAG).split("_")[0])
        if d.WEIGHTED_SR.ENABLE:
            lo, hi = d.WEIGHTED_SR.RANGES[int(self._np_rng.choice(len(d.WEIGHTED_SR.RANGES), p=d.WEIGHTED_SR.WEIGHTS))]
            return self._rng.randint(int(lo), int(hi))
        return self._rng.randint(int(d.RANDOM_RESAMPLE[0]), int(d.RANDOM_RESAMPLE[-1]))

    def _to_target_rate(self, waves, lengths, file_rates):
        """-> [(n_i) rows at the target rate]: the clips of one file rate resampled together, cut back to their own lengths."""
        rows = [None] * len(lengths)
        for sr in sorted(set(file_rates)):
            idx = [i for i, r in enumerate(file_rates) if r == sr]
            if sr == self.target_sr:
                for i in idx:
                    rows[i] = waves[i, 0, :lengths[i]]
                continue
            # a shorter clip of the group is followed by collate's zeros, which is the resampler's own padding: its first
            # ceil(n*up/down) outputs are those of the clip resampled alone
            n = max(lengths[i] for i in idx)
            out = resample.resample_poly(waves[idx, 0, :n], self.target_sr, sr)
            for j, i in enumerate(idx):
                rows[i] = out[j, :-(-lengths[i] * self.target_sr // sr)]
        return rows

    def __iter__(self):
        if self._gen is None:
            self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
        for waves, lengths, file_rates, names in self.loader:
            rows = self._to_target_rate(waves.to(self.device, non_blocking=True), lengths, file_rates)
            if self.training:
                rows = [r[:self.seg] for r in rows]
            pads = [pad_length(int(r.shape[-1]), self.seg) for r in rows]
            T = max(int(r.shape[-1]) + p for r, p in zip(rows, pads))
            pads = [T - int(r.shape[-1]) for r in rows]       # (a batch of several test clips: noise up to the longest)
            tgt = torch.empty(len(rows), T, dtype=torch.float32, device=self.device)
            if any(pads):
                tgt.normal_(generator=self._gen).mul_(self.config.DATA.PAD_WHITENOISE)
            for i, r in enumerate(rows):
                tgt[i, :r.shape[-1]] = r
            rates = [self.draw_rate() for _ in rows]
            wave_in = resample.degrade_batch(tgt, self.target_sr, rates)
            highcut = torch.tensor([resample.highcut_bin(self.config, r) for r in rates], dtype=torch.int64)
            yield wave_in.unsqueeze(1), tgt.unsqueeze(1), highcut, names, torch.tensor(pads, dtype=torch.int64)


def get_loader(config, device, logger=None, drop_last=False):
    """The reference's get_loader (data_loaders.py:25-79): (train, validation) loaders over a random split of the training clips
    (DATA.VALID_SPLIT, generator seed 42), or the test loader (batch 1, in order) with EVAL_MODE — each wrapped in PrepareOnDevice.
    `drop_last`: the training loader drops an incomplete last batch (a step replayed from a HIP graph has one batch size)."""
    if config.DATA.DATASET != "VCTK_092":
        raise NotImplementedError(f"Dataset {config.DATA.DATASET} not implemented")
    device = torch.device(device)
    kw = dict(num_workers=min(int(config.DATA.NUM_WORKERS), 16), pin_memory=device.type == "cuda", collate_fn=collate_clips)
    if config.EVAL_MODE:
        ds = WavFolder(config, training=False)
        if logger:
            logger.info(f"{len(ds)} test clips of {len(ds.speakers)} speakers in {ds.root}")
        return PrepareOnDevice(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, **kw), config, device, False, config.SEED)
    ds = WavFolder(config, training=True)
    n_train = int(len(ds) * (1 - config.DATA.VALID_SPLIT))
    train, val = torch.utils.data.random_split(ds, [n_train, len(ds) - n_train], generator=torch.Generator().manual_seed(42))
    if logger:
        logger.info(f"{len(train)} training and {len(val)} validation clips of {len(ds.speakers)} speakers in {ds.root}")
    loaders = [torch.utils.data.DataLoader(part, batch_size=config.DATA.BATCH_SIZE, shuffle=True, drop_last=drop_last and part is train, **kw)
               for part in (train, val)]
    return (PrepareOnDevice(loaders[0], config, device, True, config.SEED),
            PrepareOnDevice(loaders[1], config, device, True, config.SEED + 1))
