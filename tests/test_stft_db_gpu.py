"""The "dB" spectrogram scale on the GPU (vm_asr_amd/csrc/stft.hip: stft_like_kernel<0, 1> + db_floor_kernel, istft_frames_kernel<0, 1>,
stft_like_kernel<2, 1>) against the float64 restatement of the reference's branch (tests/stft_db_ref.py).

Gates.  Forward: the log of a nearly cancelled bin amplifies the FFT's absolute error, so no fixed dB figure; the rule for fp32 results
instead: worst |hip - f64| <= 2 x worst |f32 - f64| per tensor, f32 being the same restatement run in float32 on the CPU (two fp32
FFTs with different butterfly orders).  Inverse and gradient: the log2 tests' gates (tests/test_gpu_kernels.py::
test_stft_istft_golden: rtol 1e-4, atol 1e-5), the absolute part scaled by max(1, max|ref|).  Every case prints its figures
(pytest -s); profiles/stft_db.md keeps them."""
import os

import numpy as np
import pytest
import torch

import stft_db_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# (n_fft, hop, win, T): the smallest admitted n_fft with an even (10) and an odd (11) frame count (a workgroup owns frames in
# pairs), a window padded inside n_fft, the shortest admitted clip (T = n_fft/2 + 1, 3 frames), and the shipped transform size
GEOMETRIES = [(64, 16, 64, 150), (64, 16, 64, 160), (64, 16, 48, 150), (64, 16, 64, 33), (1024, 240, 1024, 4800)]
IDS = ["n64_even", "n64_odd", "n64_win48", "n64_shortest", "n1024"]

_cache = {}


def _case(geo, B):
    """Inputs and CPU answers of one forward case, computed once."""
    key = (geo, B)
    if key not in _cache:
        n_fft, hop, win, T = geo
        x = ref.clips(B, T, win)
        mag64, ph64, raw64 = ref.wav2spectro_db(x, n_fft, hop, win)
        mag32, _, _ = ref.wav2spectro_db(x, n_fft, hop, win, torch.float32)
        _cache[key] = (x, mag64, ph64, raw64, mag32)
    return _cache[key]


def _close(got, want, rtol, atol, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    d = (got - want).abs()
    print(f"{what}: max|diff| {d.max().item():.3e}  max|ref| {want.abs().max().item():.3e}  (rtol {rtol:g}, atol {atol:.3e})")
    assert (d - (atol + rtol * want.abs())).max().item() <= 0, f"{what}: max|diff|={d.max().item():.3e} (rtol={rtol}, atol={atol:.3e})"


def _scaled(want, tol=1e-5):
    return tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_db_forward_against_float64(geo, B):
    from vm_asr_amd import stft
    n_fft, hop, win, T = geo
    x, mag64, ph64, raw64, mag32 = _case(geo, B)
    # the inputs make both clamps work: the floor binds somewhere and leaves bins free; B = 3 has the all-zero clip on amin
    floor = raw64.amax() - 80.0
    assert (raw64 < floor).any() and (raw64 > floor).any()
    if B == 3:
        assert (raw64[1] == -100.0).all() and (mag64[1] == floor).all()
    if B >= 2:
        assert 35.0 < mag64[0].max().item() - mag64[-1].max().item() < 45.0
    mag, ph = stft.wav2spectro(x.to(DEV)[:, None], n_fft, hop, win, "dB")
    assert mag.shape == (B, 1, n_fft // 2 + 1, 1 + T // hop) and mag.dtype == torch.float32
    magf = mag[:, 0]
    assert torch.isfinite(magf).all()
    floor_dev = magf.max() - 80.0                             # fp32, as the kernel forms it from the call's own maximum
    assert torch.equal(magf.min(), floor_dev)
    on_floor = (magf == floor_dev).float().mean().item()
    mag = magf.double().cpu()
    e_hip, e_f32 = (mag - mag64).abs().max().item(), (mag32.double() - mag64).abs().max().item()
    print(f"dB forward n_fft {n_fft} hop {hop} win {win} T {T} B {B}: worst |hip - f64| {e_hip:.3e} dB, worst |f32 - f64| {e_f32:.3e} dB, "
          f"ratio {e_hip / e_f32:.2f}; on the floor {on_floor:.3f} of the bins")
    assert e_hip <= 2.0 * e_f32, (e_hip, e_f32)
    # phase: the log2 call's, bit for bit
    _, ph2 = stft.wav2spectro(x.to(DEV)[:, None], n_fft, hop, win, "log2")
    assert torch.equal(ph, ph2)


def test_db_floor_is_batch_wide_on_the_device():
    """The quiet clip alone and as a row of the joint call differ exactly where the joint floor (from the loud clip) is higher."""
    from vm_asr_amd import stft
    n_fft, hop, win, T = GEOMETRIES[0]
    x = ref.clips(2, T, win).to(DEV)
    joint, _ = stft.wav2spectro(x, n_fft, hop, win, "dB")
    alone, _ = stft.wav2spectro(x[1:], n_fft, hop, win, "dB")
    loud, _ = stft.wav2spectro(x[:1], n_fft, hop, win, "dB")
    floor = joint.max() - 80.0
    assert joint.max().item() == joint[0].max().item() and torch.equal(joint[0], loud[0])
    assert torch.equal(joint[1], torch.maximum(alone[0], floor))
    raised = alone[0] < floor
    assert torch.equal(joint[1] != alone[0], raised)
    assert raised.any() and (~raised).any()
    assert alone.min().item() < floor.item() - 15.0     # alone, the quiet clip keeps bins well below the joint floor


@pytest.mark.parametrize("geo", GEOMETRIES, ids=IDS)
def test_db_inverse_against_float64(geo):
    """mag over the range the forward produces (its floor included: a fifth of the bins sit on it), phases over the circle."""
    from vm_asr_amd import stft
    n_fft, hop, win, T = geo
    _, mag64, _, _, _ = _case(geo, 3)
    hi, lo = mag64.max().item(), mag64.min().item()
    assert abs(hi - lo - 80.0) < 1e-9
    g = torch.Generator().manual_seed(n_fft + win + T)
    shape = (3, n_fft // 2 + 1, 1 + T // hop)
    mag = (lo + (hi - lo) * torch.rand(shape, generator=g)).float()
    mag[torch.rand(shape, generator=g) < 0.2] = lo
    phase = ((2 * torch.rand(shape, generator=g) - 1) * np.pi).float()
    want = ref.spectro2wav_db(mag, phase, hop, win)
    got = stft.spectro2wav(mag.to(DEV), phase.to(DEV), n_fft, hop, win, "dB")
    assert got.shape == want.shape == (3, hop * (shape[2] - 1))
    _close(got, want, 1e-4, _scaled(want), f"dB inverse n_fft {n_fft} win {win} T {T}")


@pytest.mark.parametrize("geo", [GEOMETRIES[0], GEOMETRIES[2], GEOMETRIES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_db_round_trip_where_nothing_is_clamped(geo):
    """White noise keeps every bin within 80 dB of the loudest (checked on the restatement), so spectro2wav undoes wav2spectro."""
    from vm_asr_amd import stft
    n_fft, hop, win, T = geo
    T = (T // hop) * hop        # istft returns hop * (M - 1) samples
    g = torch.Generator().manual_seed(T)
    x = 0.1 * torch.randn(2, T, generator=g)
    mag64, _, raw64 = ref.wav2spectro_db(x, n_fft, hop, win)
    assert torch.equal(mag64, raw64) and raw64.min().item() > -100.0
    mag, ph = stft.wav2spectro(x.to(DEV), n_fft, hop, win, "dB")
    assert mag.min().item() > mag.max().item() - 80.0
    back = stft.spectro2wav(mag, ph, n_fft, hop, win, "dB")
    err = (back.cpu() - x).abs().max().item()
    print(f"dB round trip n_fft {n_fft} win {win}: max|diff| {err:.3e}")
    assert err < 1e-4 * max(1.0, x.abs().max().item())      # the log2 round trip's gate (test_stft_istft_golden)


@pytest.mark.parametrize("geo", [GEOMETRIES[1], GEOMETRIES[2], GEOMETRIES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_db_inverse_gradient_against_float64_autograd(geo):
    from vm_asr_amd.stft import ISTFTFunction
    n_fft, hop, win, T = geo
    g = torch.Generator().manual_seed(7 * n_fft + T)
    shape = (2, n_fft // 2 + 1, 1 + T // hop)
    mag = (-60.0 + 70.0 * torch.rand(shape, generator=g)).float()
    mag[torch.rand(shape, generator=g) < 0.2] = -70.0
    phase = ((2 * torch.rand(shape, generator=g) - 1) * np.pi).float()
    gw = torch.randn(2, hop * (shape[2] - 1), generator=g)
    m64, p64 = mag.double().requires_grad_(), phase.double().requires_grad_()
    ref.spectro2wav_db(m64, p64, hop, win).backward(gw.double())
    md, pd = mag.to(DEV).requires_grad_(), phase.to(DEV).requires_grad_()
    ISTFTFunction.apply(md, pd, hop, win, "dB").backward(gw.to(DEV))
    _close(md.grad, m64.grad, 1e-4, _scaled(m64.grad), f"dB dmag n_fft {n_fft} win {win}")
    _close(pd.grad, p64.grad, 1e-4, _scaled(p64.grad), f"dB dphase n_fft {n_fft} win {win}")
    # the scale reaches the backward: under log2 the same call differentiates 2^mag
    m2, p2 = mag.to(DEV).requires_grad_(), phase.to(DEV).requires_grad_()
    ISTFTFunction.apply(m2, p2, hop, win).backward(gw.to(DEV))
    assert (m2.grad - md.grad).abs().max().item() > 0


def test_db_calls_are_bit_reproducible():
    from vm_asr_amd import stft
    n_fft, hop, win, T = GEOMETRIES[4]
    x = ref.clips(3, T, win).to(DEV)
    a, b = stft.wav2spectro(x, n_fft, hop, win, "dB"), stft.wav2spectro(x, n_fft, hop, win, "dB")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    gw = torch.randn(3, hop * (a[0].shape[-1] - 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    grads = []
    for _ in range(2):
        m, p = a[0].clone().requires_grad_(), a[1].clone().requires_grad_()
        w = stft.spectro2wav(m, p, n_fft, hop, win, "dB")
        w.backward(gw)
        grads.append((w.detach(), m.grad, p.grad))
    for u, v in zip(*grads):
        assert torch.equal(u, v)


def test_log2_path_still_matches_its_fixture():
    """wav2spectro / spectro2wav under "log2" against tests/golden/stft.npz, under the gates of
    tests/test_gpu_kernels.py::test_stft_istft_golden (the scaled entry points with the log2 code are what Python calls now)."""
    from vm_asr_amd import stft
    z = np.load(os.path.join(GOLDEN, "stft.npz"))

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).float()

    for k in "stwr":
        n_fft, hop, win = (int(v) for v in z[f"{k}_cfg"])
        mag, _ = stft.wav2spectro(t(z[f"{k}_wav"]), n_fft, hop, win, "log2")
        _close(mag, torch.from_numpy(z[f"{k}_mag"]), 1e-4, 2e-4, f"log2 {k} mag")
        m2, p2 = t(z[f"{k}_imag"]).requires_grad_(), t(z[f"{k}_iphase"]).requires_grad_()
        rec = stft.spectro2wav(m2, p2, n_fft, hop, win, "log2")
        _close(rec, torch.from_numpy(z[f"{k}_rec"]), 1e-4, 1e-5, f"log2 {k} rec")
        rec.backward(t(z[f"{k}_grec"]))
        _close(m2.grad, torch.from_numpy(z[f"{k}_dmag"]), 1e-4, _scaled(torch.from_numpy(z[f"{k}_dmag"])), f"log2 {k} dmag")
        _close(p2.grad, torch.from_numpy(z[f"{k}_dphase"]), 1e-4, _scaled(torch.from_numpy(z[f"{k}_dphase"])), f"log2 {k} dphase")
        # the first entry points (kept for C callers) run the same kernels: the same bits
        from vm_asr_amd import _lib
        lib = _lib.lib()
        Bn, F, M = int(np.prod(m2.shape[:-2])), m2.shape[-2], m2.shape[-1]
        mm, pp = m2.detach().reshape(Bn, F, M).contiguous(), p2.detach().reshape(Bn, F, M).contiguous()
        wav = torch.empty((Bn, hop * (M - 1)), dtype=torch.float32, device=DEV)
        wsb = lib.vmasr_istft_workspace(Bn, F, M, hop)
        ws = torch.empty(wsb // 4, dtype=torch.float32, device=DEV)
        _lib.call(lib.vmasr_istft, mm, pp, wav, Bn, F, M, hop, win, ws, wsb)
        assert torch.equal(wav.view(rec.shape), rec.detach())


def test_db_forward_replays_in_a_hip_graph_on_new_input():
    """One capture (a single stream, two launches), two replays; the second sees another input and must give its answer, the
    call-wide maximum included: nothing of the floor is decided on the host."""
    from vm_asr_amd import stft
    n_fft, hop, win, T = 128, 32, 128, 2016
    x1 = ref.clips(3, T, win).to(DEV)
    x2 = (0.1 * ref.clips(3, T, win, seed=1)).to(DEV).flip(0).contiguous()      # the loud clip last and 20 dB down: another maximum
    want1, want2 = stft.wav2spectro(x1, n_fft, hop, win, "dB"), stft.wav2spectro(x2, n_fft, hop, win, "dB")
    assert abs(want1[0].max().item() - want2[0].max().item()) > 15.0 and want2[0].max().item() - 80.0 > -100.0
    buf = x1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stft.wav2spectro(buf, n_fft, hop, win, "dB")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mag, ph = stft.wav2spectro(buf, n_fft, hop, win, "dB")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mag, want1[0]) and torch.equal(ph, want1[1])
    buf.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(mag, want2[0]) and torch.equal(ph, want2[1])
    assert torch.equal(mag.min(), want2[0].max() - 80.0)


def _tiny_generator(scale):
    from vm_asr_amd.model import DualStreamInteractiveMambaUNet
    torch.manual_seed(123)
    return DualStreamInteractiveMambaUNet(in_chans=1, patch_size=4, depths=[2, 2, 2, 2], dims=8, ssm_d_state=1, forward_type="v5",
                                          output_version="v3", concat_skip=True, interact="dual", n_fft=128, hop_length=32,
                                          win_length=128, spectro_scale=scale, low_freq_replacement=True, drop_path_rate=0.0).to(DEV)


def test_tiny_generator_runs_forward_and_backward_under_db():
    gen = _tiny_generator("dB")
    g = torch.Generator().manual_seed(5)
    wave = (0.1 * torch.randn(2, 1, 32 * 63, generator=g)).to(DEV)
    hf = torch.full((2,), 21, dtype=torch.int64, device=DEV)
    y = gen(wave, hf)
    assert y.shape == wave.shape and torch.isfinite(y).all()
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    # every parameter that takes part in the forward (some of the architecture's never do, under either scale: the same set)
    log2 = _log2_grads()
    used = [(n, p) for n, p in gen.named_parameters() if p.grad is not None]
    assert len(used) > 100 and {n for n, _ in used} == {n for n, v in log2.items() if v is not None}
    for n, p in used:
        assert torch.isfinite(p.grad).all(), n
        assert p.grad.abs().max().item() > 0 or log2[n] == 0, n


def _log2_grads():
    gen = _tiny_generator("log2")
    g = torch.Generator().manual_seed(5)
    wave = (0.1 * torch.randn(2, 1, 32 * 63, generator=g)).to(DEV)
    y = gen(wave, torch.full((2,), 21, dtype=torch.int64, device=DEV))
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    return {n: None if p.grad is None else p.grad.abs().max().item() for n, p in gen.named_parameters()}


def test_one_eager_trainer_step_from_a_db_config():
    import vm_asr_amd
    from vm_asr_amd.config import get_default_config, update_config
    from vm_asr_amd.trainer import Trainer, build_optimizer
    c = get_default_config()
    c.MODEL.NAME = "DualStreamInteractiveMambaUNet"
    c.MODEL.VSSM.DIMS = 8
    c.MODEL.VSSM.DROP_PATH_RATE = 0.0
    c.DATA.STFT.N_FFT = 128
    c.DATA.STFT.WIN_LENGTH = 128
    c.DATA.STFT.SCALE = "dB"
    c.DATA.TARGET_SR = 16000           # -> hop 80
    c.DATA.SEGMENT = 80 * 63 / 16000   # 64 frames
    c.DATA.BATCH_SIZE = 2
    c.TRAIN.LOW_FREQ_REPLACEMENT = True
    c.TRAIN.ADVERSARIAL.ENABLE = True
    c.TRAIN.ADVERSARIAL.DISCRIMINATORS = ["mpd"]
    c.TRAIN.ADVERSARIAL.MPD_HIDDEN = 2
    cfg = update_config(c)
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    assert models["generator"].spectro_scale == "dB"
    opts = {"generator": build_optimizer(cfg, models["generator"]), "discriminator": build_optimizer(cfg, [models["mpd"]])}
    tr = Trainer(models, [], opts, cfg, torch.device("cuda", 0), None, None, {}, amp=False, gan=True, len_epoch=0)
    for m in tr.models.values():
        m.train()
    T = int(cfg.DATA.SEGMENT * cfg.DATA.TARGET_SR)
    g = torch.Generator().manual_seed(0)
    batch = (0.1 * torch.randn(2, 1, T, generator=g), 0.1 * torch.randn(2, 1, T, generator=g), torch.full((2,), 21, dtype=torch.int64))
    before = {k: v.detach().clone() for k, v in tr.models["generator"].state_dict().items()}
    out, logs = tr.train_step(*[t.to(DEV) for t in batch])
    assert logs and all(torch.isfinite(torch.as_tensor(v)).all() for v in logs.values()), logs
    assert torch.isfinite(out).all()
    after = tr.models["generator"].state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
