"""Wav-file inference (vm_asr_amd/inferencer.py, main.py --inference): wav decoding, padding and the highcut rule as host
logic; on the GPU a file through resample -> pad -> generator -> fold -> 16-bit wav against the same steps composed by hand.

Tiny config of tests/test_metric_fused.py: DIMS 8, N_FFT 128, 16 kHz target, 5040-sample segment; TAG 8000_16000."""
import glob
import os
import struct
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 5040


def _tiny_config(output, tag="8000_16000"):
    from vm_asr_amd.config import get_default_config, update_config
    c = get_default_config()
    c.MODEL.NAME = "DualStreamInteractiveMambaUNet"
    c.MODEL.VSSM.DIMS = 8
    c.MODEL.VSSM.DROP_PATH_RATE = 0.0
    c.DATA.STFT.N_FFT = 128
    c.DATA.STFT.WIN_LENGTH = 128
    c.DATA.TARGET_SR = 16000           # -> hop 80
    c.DATA.SEGMENT = 80 * 63 / 16000   # 5040 samples
    c.TRAIN.LOW_FREQ_REPLACEMENT = True
    c.TRAIN.ADVERSARIAL.ENABLE = False
    c.OUTPUT = str(output)
    c.TAG = tag
    return update_config(c)


def _write_wav(path, samples, sr, width=2):
    """samples: int array (T,) or (T, channels), written as they are"""
    a = np.asarray(samples)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if a.ndim == 1 else a.shape[1])
        f.setsampwidth(width)
        f.setframerate(sr)
        f.writeframes(a.astype({1: np.uint8, 2: "<i2", 4: "<i4"}[width]).tobytes())


def _pcm(n, seed, amp=6000):
    return np.random.default_rng(seed).integers(-amp, amp, size=n).astype(np.int16)


def _read_pcm(path):
    with wave.open(str(path), "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int64), f.getframerate()


def _cpu_inferencer(tmp_path, **kw):
    from vm_asr_amd.inferencer import Inferencer
    return Inferencer({"generator": torch.nn.Identity()}, _tiny_config(tmp_path / "out"), torch.device("cpu"), **kw)


# ---- CPU: host logic ---------------------------------------------------------------------------------------------------------------
def test_read_wav_scales_and_keeps_channels(tmp_path):
    from vm_asr_amd.inferencer import read_wav
    st = np.stack([_pcm(50, 0), _pcm(50, 1)], axis=1)
    st[0] = (-32768, 32767)
    _write_wav(tmp_path / "st.wav", st, 44100)
    a, sr = read_wav(str(tmp_path / "st.wav"))
    assert sr == 44100 and a.shape == (2, 50) and a.dtype == torch.float32
    assert torch.equal(a, torch.from_numpy(st.T.astype(np.float32) / 32768.0))
    assert a[0, 0] == -1.0 and a[1, 0] == 32767 / 32768
    # other integer widths the standard library opens: unsigned 8-bit, 24-bit, 32-bit
    _write_wav(tmp_path / "u8.wav", [0, 128, 255], 8000, width=1)
    assert read_wav(str(tmp_path / "u8.wav"))[0].tolist() == [[-1.0, 0.0, 127 / 128]]
    with wave.open(str(tmp_path / "s24.wav"), "wb") as f:
        f.setnchannels(1), f.setsampwidth(3), f.setframerate(8000)
        f.writeframes(b"".join(struct.pack("<i", v)[:3] for v in (-8388608, -1, 0, 8388607)))
    assert read_wav(str(tmp_path / "s24.wav"))[0].tolist() == [[-1.0, -1 / 8388608, 0.0, 8388607 / 8388608]]
    _write_wav(tmp_path / "s32.wav", [-2 ** 31, 2 ** 30], 8000, width=4)
    assert read_wav(str(tmp_path / "s32.wav"))[0].tolist() == [[-1.0, 0.5]]


def test_non_pcm_files_are_rejected(tmp_path):
    from vm_asr_amd.inferencer import read_wav
    data = np.zeros(16, dtype="<f4").tobytes()          # IEEE-float wav (format tag 3)
    fmt = struct.pack("<HHIIHH", 3, 1, 16000, 64000, 4, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    (tmp_path / "float.wav").write_bytes(b"RIFF" + struct.pack("<I", len(riff)) + riff)
    (tmp_path / "text.wav").write_text("not audio")
    for name in ("float.wav", "text.wav"):
        with pytest.raises(ValueError, match="16-bit PCM"):
            read_wav(str(tmp_path / name))
    inf = _cpu_inferencer(tmp_path)
    with pytest.raises(ValueError, match="16-bit PCM"):
        inf.load_input(str(tmp_path / "float.wav"))
    with pytest.raises(FileNotFoundError):
        inf.infer_file(str(tmp_path / "missing.wav"))


def test_load_input_stereo_mean_padding_and_highcut(tmp_path):
    inf = _cpu_inferencer(tmp_path)
    assert inf.num_frames_per_seg == SEG and (inf.input_sr, inf.target_sr) == (8000, 16000)
    st = np.stack([_pcm(1000, 2), _pcm(1000, 3)], axis=1)
    _write_wav(tmp_path / "short.wav", st, 16000)
    torch.manual_seed(11)
    w, hc, pad = inf.load_input(str(tmp_path / "short.wav"))
    assert w.shape == (1, 1, SEG) and pad == SEG - 1000
    mean = torch.from_numpy(st.astype(np.float32) / 32768.0).mean(dim=1)
    assert torch.equal(w[0, 0, :1000], mean)
    torch.manual_seed(11)
    noise = torch.randn(pad) * inf.config.DATA.PAD_WHITENOISE            # the reference's white-noise tail, same generator
    assert torch.equal(w[0, 0, 1000:], noise) and float(noise.abs().max()) > 0.0
    # a file at the target rate says nothing about its band: TAG's input rate decides
    assert hc.dtype == torch.int64 and hc.tolist() == [int(65 * 8000 / 16000)] == [32]
    # ragged: padded to the next multiple; exact multiples and one exact segment: no pad
    _write_wav(tmp_path / "ragged.wav", _pcm(2 * SEG + 100, 4), 16000)
    w, _, pad = inf.load_input(str(tmp_path / "ragged.wav"))
    assert w.shape == (1, 1, 3 * SEG) and pad == SEG - 100
    _write_wav(tmp_path / "exact.wav", _pcm(2 * SEG, 5), 16000)
    w, _, pad = inf.load_input(str(tmp_path / "exact.wav"))
    assert w.shape == (1, 1, 2 * SEG) and pad == 0
    assert [inf.pad_length(n) for n in (1, SEG - 1, SEG, SEG + 1, 3 * SEG)] == [SEG - 1, 1, 0, SEG - 1, 0]
    # the highcut rule: the file's own rate below the target rate, TAG's otherwise
    assert inf.highcut_for(8000) == 32 and inf.highcut_for(4000) == 16 and inf.highcut_for(12000) == 48
    assert inf.highcut_for(16000) == 32 and inf.highcut_for(44100) == 32
    # a file at another rate is resampled on the device: there is no CPU path
    _write_wav(tmp_path / "low.wav", _pcm(500, 6), 8000)
    with pytest.raises(RuntimeError, match="no CPU path"):
        inf.load_input(str(tmp_path / "low.wav"))


def test_input_rate_must_lie_within_random_resample(tmp_path):
    from vm_asr_amd.inferencer import Inferencer
    with pytest.raises(ValueError, match="Input sampling rate mismatch"):
        Inferencer({"generator": torch.nn.Identity()}, _tiny_config(tmp_path, tag="1000_16000"), torch.device("cpu"))
    with pytest.raises(ValueError, match="TAG"):
        Inferencer({"generator": torch.nn.Identity()}, _tiny_config(tmp_path, tag="untagged"), torch.device("cpu"))


def test_main_inference_is_built(tmp_path):
    """--inference used to end in SystemExit("--inference is not built ..."): the flag now leads to the inferencer (which asks for
    --input before it needs a GPU)."""
    sys.path.insert(0, ROOT)
    import main
    cfg = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "configs", "vm_asr_16k*.yaml")))[0]
    args, config = main.parse_option(["--cfg", cfg, "--inference", "--tag", "8000_16000", "--output", str(tmp_path)])
    assert config.INFERENCE_MODE and args.input is None and args.segment_batch == 1 and args.degrade is False
    with pytest.raises(SystemExit) as e:
        main.main(args, config)
    assert "not built" not in str(e.value) and "--input" in str(e.value)
    assert "not built" not in open(os.path.join(ROOT, "main.py")).read()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _gpu_inferencer(tmp_path, segment_batch=1):
    import vm_asr_amd
    from vm_asr_amd.inferencer import Inferencer
    cfg = _tiny_config(tmp_path / "out")
    torch.manual_seed(cfg.SEED)
    gen = vm_asr_amd.get_model(cfg)["generator"]
    return Inferencer({"generator": gen}, cfg, torch.device("cuda:0"), segment_batch=segment_batch), cfg


@pytest.mark.gpu
def test_infer_file_matches_the_composition_by_hand(tmp_path):
    from vm_asr_amd import resample
    from vm_asr_amd.tester import Tester
    inf, cfg = _gpu_inferencer(tmp_path)
    n8 = SEG + 130                                   # 8 kHz mono -> 10 340 samples at 16 kHz: three ragged segments
    pcm = _pcm(n8, 7)
    _write_wav(tmp_path / "clip.wav", pcm, 8000)
    torch.manual_seed(3)
    out = inf.infer_file(str(tmp_path / "clip.wav"), str(tmp_path / "enh"))
    got, sr = _read_pcm(tmp_path / "enh" / "clip_enhanced.wav")
    assert sr == 16000 and got.shape == (2 * n8,) and out.shape == (1, 1, 2 * n8)
    assert not os.path.exists(os.path.join(cfg.OUTPUT, "clip_enhanced.wav"))          # output_dir is honoured
    # by hand: resample_poly -> white-noise pad -> Tester._enhance (the evaluation path's segment loop) -> 16-bit
    torch.manual_seed(3)
    x = torch.from_numpy(pcm.astype(np.float32) / 32768.0).cuda().view(1, -1)
    up = resample.resample_poly(x, 16000, 8000)
    pad = 3 * SEG - up.shape[-1]
    assert up.shape[-1] == 2 * n8 and 0 < pad < SEG
    padded = torch.cat((up, (torch.randn(pad) * cfg.DATA.PAD_WHITENOISE).unsqueeze(0).cuda()), dim=-1).unsqueeze(0)
    tester = Tester({"generator": inf.models["generator"]}, [], cfg, torch.device("cuda:0"), None)
    with torch.no_grad():
        want = tester._enhance(padded, torch.tensor([32], dtype=torch.int64))
    assert want.shape == (1, 1, 3 * SEG)
    want16 = (want[0, 0, :2 * n8].float().clamp(-1, 1) * 32767.0).round().cpu().numpy().astype(np.int64)
    assert np.abs(got - want16).max() <= 1
    assert np.abs(got).max() > 100                   # a signal, not silence
    # four segments per generator call: the same file within one LSB
    inf4, _ = _gpu_inferencer(tmp_path, segment_batch=4)
    torch.manual_seed(3)
    inf4.infer_file(str(tmp_path / "clip.wav"), str(tmp_path / "enh4"))
    got4, _ = _read_pcm(tmp_path / "enh4" / "clip_enhanced.wav")
    assert got4.shape == got.shape and np.abs(got4 - got).max() <= 1


@pytest.mark.gpu
def test_single_segment_takes_the_direct_path_and_directory_lists_outputs(tmp_path, monkeypatch):
    from vm_asr_amd import tester
    inf, cfg = _gpu_inferencer(tmp_path)
    src = tmp_path / "clips"
    src.mkdir()
    _write_wav(src / "b.wav", _pcm(1200, 8), 8000)          # 2400 samples at 16 kHz: one padded segment
    _write_wav(src / "a.wav", _pcm(SEG, 9), 16000)          # exactly one segment at the target rate
    (src / "notes.txt").write_text("skipped")

    def no_unfold(*a, **k):
        raise AssertionError("a single segment must not be unfolded")
    monkeypatch.setattr(tester, "unfold_audio", no_unfold)
    calls, gen = [], inf.models["generator"]
    handle = gen.register_forward_hook(lambda m, args, out: calls.append(tuple(args[0].shape)))
    written = inf.infer_directory(str(src))
    handle.remove()
    assert calls == [(1, 1, SEG), (1, 1, SEG)]
    want = [os.path.join(cfg.OUTPUT, "clips", "a_enhanced.wav"), os.path.join(cfg.OUTPUT, "clips", "b_enhanced.wav")]
    assert written == want and all(os.path.isfile(p) for p in want)
    assert _read_pcm(want[0])[0].shape == (SEG,) and _read_pcm(want[1])[0].shape == (2400,)
    assert _read_pcm(want[1])[1] == 16000
    assert inf.infer_directory(str(src), str(tmp_path / "elsewhere"), file_types=(".flac",)) == []
