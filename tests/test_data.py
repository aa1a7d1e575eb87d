"""The wav-folder data pipeline's host side (vm_asr_amd/data.py, main.py --data-path): listing and splits of WavFolder, decoding
rules, collation, the rate draws of PrepareOnDevice and the command line.  Nothing here needs a GPU; the device half is
tests/test_datapipe_gpu.py.
"""
import os
import random
import struct
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 2048


def write_wav(path, data, sr):
    """data (n,) or (n, channels) float in [-1, 1) -> 16-bit PCM."""
    data = np.asarray(data, dtype=np.float64)
    pcm = np.round(data * 32767.0).astype("<i2")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def make_config(data_path, **data):
    from vm_asr_amd.config import get_config
    cfg = get_config(opts=["DATA.TARGET_SR", 48000], tag="16000_48000")
    cfg.defrost()
    cfg.DATA.DATA_PATH, cfg.DATA.FLAC2WAV.DST_PATH = str(data_path), "wavs"
    cfg.DATA.SEGMENT = (SEG + 0.5) / 48000          # int(SEGMENT * 48000) == SEG
    cfg.DATA.TRAIN_SPLIT, cfg.DATA.USE_QUANTITY, cfg.DATA.BATCH_SIZE = [2, 1], 1.0, 2
    for k, v in data.items():
        setattr(cfg.DATA, k, v)
    cfg.freeze()
    return cfg


# name -> (rate, frames, channels): mono and stereo, one file at 16 kHz, one shorter than a segment
FILES = {"p1_001.wav": (48000, 3000, 1), "p1_002.wav": (48000, 1000, 2), "p2_001.wav": (16000, 2500, 1), "p2_002.wav": (48000, 2048, 2),
         "p3_001.wav": (48000, 5000, 1), "p3_002.wav": (48000, 700, 1)}


def make_folder(tmp_path):
    """-> {name: decoded (channels, n) float32} of FILES written below tmp_path/wavs/<speaker>/."""
    rng = np.random.default_rng(5)
    out = {}
    for name, (sr, n, ch) in FILES.items():
        data = 0.1 * rng.standard_normal((n, ch) if ch > 1 else n)
        got = write_wav(os.path.join(str(tmp_path), "wavs", name[:2], name), data, sr)
        out[name] = got.reshape(n, ch).T
    return out


def test_wavfolder_splits_speakers_and_keeps_a_seeded_quantity(tmp_path):
    from vm_asr_amd.data import WavFolder
    make_folder(tmp_path)
    cfg = make_config(tmp_path)
    train, test = WavFolder(cfg, training=True), WavFolder(cfg, training=False)
    assert train.speakers == ["p1", "p2"] and test.speakers == ["p3"]
    assert sorted(n for _, n in train.ids) == ["p1_001.wav", "p1_002.wav", "p2_001.wav", "p2_002.wav"]
    assert [n for _, n in test.ids] == ["p3_001.wav", "p3_002.wav"]                  # in order, all of them
    half = WavFolder(make_config(tmp_path, USE_QUANTITY=0.5), training=True)
    want = [(s, f) for s in ("p1", "p2") for f in (f"{s}_001.wav", f"{s}_002.wav")]
    random.Random(cfg.SEED).shuffle(want)
    assert half.ids == want[:2] and half.ids == WavFolder(make_config(tmp_path, USE_QUANTITY=0.5), training=True).ids
    assert len(WavFolder(make_config(tmp_path, USE_QUANTITY=0.5), training=False)) == 2   # the quantity is a training matter
    assert len(WavFolder(cfg, training=True, root=os.path.join(str(tmp_path), "wavs"))) == 4
    with pytest.raises(ValueError, match="sox"):
        WavFolder(make_config(tmp_path, RESAMPLER="sox"), training=True)
    with pytest.raises(FileNotFoundError):
        WavFolder(make_config(tmp_path / "absent"), training=True)


def test_wavfolder_items_first_frames_mono_cpu(tmp_path):
    from vm_asr_amd.data import WavFolder
    decoded = make_folder(tmp_path)
    cfg = make_config(tmp_path)
    train, test = WavFolder(cfg, training=True), WavFolder(cfg, training=False)
    seen = {}
    for i in range(len(train)):
        w, sr, name = train[i]
        seen[name] = w
        assert w.device.type == "cpu" and w.dtype == torch.float32 and sr == FILES[name][0]
        n = min(FILES[name][1], SEG)                                                    # the first int(SEGMENT * SRC_SR) frames
        assert w.shape == (1, n)
        assert torch.equal(w, torch.from_numpy(decoded[name][:, :n]).mean(dim=0, keepdim=True))
    assert seen["p1_002.wav"].shape == (1, 1000) and seen["p2_001.wav"].shape == (1, SEG)
    w, sr, name = test[0]
    assert name == "p3_001.wav" and w.shape == (1, 5000)                                # testing: the whole file


def test_a_file_that_is_not_pcm_names_its_path(tmp_path):
    from vm_asr_amd.data import WavFolder
    make_folder(tmp_path)
    bad = os.path.join(str(tmp_path), "wavs", "p3", "p3_000.wav")
    with open(bad, "wb") as f:          # WAVE_FORMAT_IEEE_FLOAT: the standard library refuses it
        body = struct.pack("<4sIHHIIHH", b"fmt ", 16, 3, 1, 48000, 48000 * 4, 4, 32) + struct.pack("<4sI", b"data", 16) + bytes(16)
        f.write(struct.pack("<4sI4s", b"RIFF", 4 + len(body), b"WAVE") + body)
    ds = WavFolder(make_config(tmp_path), training=False)
    assert ds.ids[0][1] == "p3_000.wav"
    with pytest.raises(ValueError, match="p3_000.wav"):
        ds[0]


def test_collate_clips_pads_and_keeps_lengths_and_rates():
    from vm_asr_amd.data import collate_clips
    a, b = torch.arange(1, 6, dtype=torch.float32).view(1, 5), torch.arange(1, 4, dtype=torch.float32).view(1, 3)
    waves, lengths, rates, names = collate_clips([(a, 48000, "a.wav"), (b, 16000, "b.wav")])
    assert waves.shape == (2, 1, 5) and lengths == [5, 3] and rates == [48000, 16000] and names == ["a.wav", "b.wav"]
    assert torch.equal(waves[0], a) and torch.equal(waves[1, :, :3], b) and not waves[1, :, 3:].any()


def test_pad_length_is_the_references():
    from vm_asr_amd.data import pad_length
    assert [pad_length(n, 100) for n in (1, 99, 100, 101, 200, 250)] == [99, 1, 0, 99, 0, 50]


def test_rate_draws(tmp_path):
    from vm_asr_amd.data import PrepareOnDevice
    cfg = make_config(tmp_path)
    p = PrepareOnDevice([], cfg, "cpu", training=True, seed=7)
    draws = [p.draw_rate() for _ in range(1000)]
    rng = random.Random(7)
    assert draws == [rng.randint(8000, 48000) for _ in range(1000)]                     # one stream of random.Random(seed)
    assert min(draws) >= 8000 and max(draws) <= 48000 and len(set(draws)) > 900
    ranges, weights = [[8000, 9000], [20000, 21000], [40000, 48000]], [0.5, 0.3, 0.2]
    cfgw = make_config(tmp_path)
    cfgw.defrost()
    cfgw.DATA.WEIGHTED_SR.ENABLE, cfgw.DATA.WEIGHTED_SR.RANGES, cfgw.DATA.WEIGHTED_SR.WEIGHTS = True, ranges, weights
    cfgw.freeze()
    pw = PrepareOnDevice([], cfgw, "cpu", training=True, seed=7)
    draws = [pw.draw_rate() for _ in range(1000)]
    rng, nrng = random.Random(7), np.random.default_rng(7)
    want = []
    for _ in range(1000):
        lo, hi = ranges[int(nrng.choice(3, p=weights))]
        want.append(rng.randint(lo, hi))
    assert draws == want
    share = [sum(lo <= d <= hi for d in draws) / 1000.0 for lo, hi in ranges]
    assert sum(share) == 1.0                                                            # every draw inside one of the ranges
    assert all(abs(s - w) < 0.06 for s, w in zip(share, weights)), share               # 4 sigma of a binomial share at n = 1000
    pe = PrepareOnDevice([], cfg, "cpu", training=False, seed=7)
    assert [pe.draw_rate() for _ in range(5)] == [16000] * 5 and pe.target_sr == 48000   # evaluation: TAG's rates


def test_main_takes_data_path_and_refuses_it_with_synthetic(tmp_path, capsys):
    import sys
    sys.path.insert(0, ROOT)
    import main
    yml = os.path.join(ROOT, "tests", "golden", "configs", "vm_asr_48k.yaml")
    args, config = main.parse_option(["--cfg", yml, "--data-path", str(tmp_path), "--output", str(tmp_path)])
    assert args.data_path == str(tmp_path) and config.DATA.DATA_PATH == str(tmp_path)
    args, config = main.parse_option(["--cfg", yml, "--output", str(tmp_path)])
    assert args.data_path is None and args.synthetic == 64 and config.DATA.DATA_PATH != str(tmp_path)      # as before
    assert main.parse_option(["--cfg", yml, "--synthetic", "8", "--output", str(tmp_path)])[0].synthetic == 8
    with pytest.raises(SystemExit):
        main.parse_option(["--cfg", yml, "--data-path", str(tmp_path), "--synthetic", "8"])
    assert "exclude each other" in capsys.readouterr().err


def test_get_loader_follows_the_reference(tmp_path):
    from vm_asr_amd import data
    make_folder(tmp_path)
    cfg = make_config(tmp_path, VALID_SPLIT=0.25, NUM_WORKERS=0)
    train, val = data.get_loader(cfg, "cpu")
    assert isinstance(train, data.PrepareOnDevice) and train.training and val.training
    assert len(train.loader.dataset) == 3 and len(val.loader.dataset) == 1 and train.loader.batch_size == 2
    parts = torch.utils.data.random_split(range(4), [3, 1], generator=torch.Generator().manual_seed(42))
    assert list(train.loader.dataset.indices) == list(parts[0].indices)                 # random_split, generator seed 42
    assert isinstance(train.loader.sampler, torch.utils.data.RandomSampler) and train.loader.collate_fn is data.collate_clips
    big = make_config(tmp_path, NUM_WORKERS=64)
    assert data.get_loader(big, "cpu")[0].loader.num_workers == 16
    cfg.defrost()
    cfg.EVAL_MODE = True
    cfg.freeze()
    test = data.get_loader(cfg, "cpu")
    assert not test.training and test.loader.batch_size == 1 and isinstance(test.loader.sampler, torch.utils.data.SequentialSampler)
    assert len(test) == 2


def test_prepare_on_a_cpu_device_raises_at_the_first_batch(tmp_path):
    from vm_asr_amd import data
    make_folder(tmp_path)
    cfg = make_config(tmp_path, NUM_WORKERS=0)
    ds = data.WavFolder(cfg, training=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=data.collate_clips)
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(iter(data.PrepareOnDevice(loader, cfg, "cpu", training=True)))
