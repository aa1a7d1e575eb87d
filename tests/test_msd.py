"""The multi-scale discriminator on the host: module, losses, trainer wiring and checkpoints against the reference's goldens
(tests/golden/msd.npz, trainstep_msd.npz), the VMASR_MSD_CONV switch and the C ABI's argument checks (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from msd_common import GOLDEN, fixture_state, load_msd, make_trainer, run_eval, check_trainstep  # noqa: F401


def _config(discs):
    from vm_asr_amd.config import get_default_config, update_config
    c = get_default_config()
    c.TRAIN.ADVERSARIAL.ENABLE = True
    c.TRAIN.ADVERSARIAL.DISCRIMINATORS = list(discs)
    c.TRAIN.ADVERSARIAL.MPD_HIDDEN = 2
    return update_config(c)


def test_get_model_builds_both_discriminators():
    """The reference builds MultiScaleDiscriminator() (hidden 128; it has no config field for the width), the fixture holds hidden 16:
    same key list; the shapes are those of the reference's layer table at each width, and at 16 they are the fixture's."""
    import vm_asr_amd
    from vm_asr_amd.msd import MultiScaleDiscriminator
    models = vm_asr_amd.get_model(_config(["mpd", "msd"]))
    assert list(models) == ["generator", "mpd", "msd"] and models["mpd"] is not None
    z = np.load(f"{GOLDEN}/msd.npz")
    keys, shapes, _ = fixture_state(z)
    sd = models["msd"].state_dict()
    assert list(sd.keys()) == keys
    small = MultiScaleDiscriminator(hidden=16).state_dict()
    assert list(small.keys()) == keys and {k: tuple(v.shape) for k, v in small.items()} == shapes
    def spec(h):     # model/discriminator.py:181-258: (Cin, Cout, k, groups) of convs.0-6 and conv_post
        layers = [(1, h, 15, 1), (h, h, 41, 4), (h, 2 * h, 41, 16), (2 * h, 4 * h, 41, 16), (4 * h, 8 * h, 41, 16), (8 * h, 8 * h, 41, 16),
                  (8 * h, 8 * h, 5, 1), (8 * h, 1, 3, 1)]
        out = {}
        for i in range(3):
            for j, (ci, co, k, g) in enumerate(layers):
                name = f"discriminators.{i}." + (f"convs.{j}" if j < 7 else "conv_post")
                out[name + ".bias"] = (co,)
                out[name + ".parametrizations.weight.original"] = (co, ci // g, k)
                out[name + ".parametrizations.weight.0._u"] = (co,)
                out[name + ".parametrizations.weight.0._v"] = (ci // g * k,)
        return out
    assert spec(16) == shapes
    assert {k: tuple(v.shape) for k, v in sd.items()} == spec(128)


def test_reference_state_dict_loads_strict():
    load_msd("cpu")


def test_msd_eval_train_cpu():
    """Eval-mode scores, 48 feature maps, three losses, three gradients, then u / v after one train-mode forward: the tolerance
    tests/test_mpd.py::test_mpd_eval_cpu holds the MPD to (2e-5 of each tensor's max; 5x that for gradients)."""
    run_eval("cpu", 2e-5)


def test_msd_forward_variants_cpu():
    """forward_pair / forward_single give forward()'s results; y_hat=None gives zeros in the generated lists."""
    z, D = load_msd("cpu")
    D.eval()
    y, y_hat = torch.from_numpy(z["y"]), torch.from_numpy(z["y_hat"])
    with torch.no_grad():
        rs, gs, fr, fg = D(y, y_hat)
        prs, pgs, pfr, pfg = D.forward_pair(y, y_hat)
        ss, sf = D.forward_single(y_hat, detach_weights=True)
        nrs, ngs, nfr, nfg = D(y, None)
    assert ngs == [0, 0, 0] and nfg == [0, 0, 0]
    for i in range(3):
        assert torch.allclose(rs[i], prs[i], rtol=1e-5, atol=1e-6) and torch.allclose(gs[i], pgs[i], rtol=1e-5, atol=1e-6)
        assert torch.equal(gs[i], ss[i]) and torch.equal(rs[i], nrs[i])
        for j in range(8):
            assert torch.allclose(fr[i][j], pfr[i][j], rtol=1e-5, atol=1e-6) and torch.equal(fg[i][j], sf[i][j])


def test_trainer_losses_vs_reference_cpu():
    from oracle.torch_backend import oracle_stft_patch
    with oracle_stft_patch():
        check_trainstep("cpu")


@pytest.mark.parametrize("discs", [("msd",), ("mpd", "msd")])
def test_eager_step_moves_msd_parameters_cpu(discs):
    from oracle.torch_backend import oracle_stft_patch
    with oracle_stft_patch():
        z, tr = make_trainer("cpu", discs)
        before = {k: v.detach().clone() for k, v in tr.models["msd"].named_parameters()}
        wave_target = torch.from_numpy(z["wave_target"])
        hf = torch.full((2,), 171, dtype=torch.int64)
        _, logs = tr.train_step(wave_target, wave_target, hf)
    assert "generator/adversarial_msd" in logs and "generator/features_msd" in logs
    assert ("generator/adversarial_mpd" in logs) == ("mpd" in discs)
    moved = 0
    for k, v in tr.models["msd"].named_parameters():
        assert torch.isfinite(v).all(), k
        moved += int(not torch.equal(v, before[k]))
    assert moved == len(before)
    assert all(np.isfinite(float(v)) for v in logs.values())


def test_checkpoint_round_trip_restores_msd(tmp_path):
    from oracle.torch_backend import oracle_stft_patch
    with oracle_stft_patch():
        z, tr = make_trainer("cpu", output=tmp_path)
        wave_target = torch.from_numpy(z["wave_target"])
        tr.train_step(wave_target, wave_target, torch.full((2,), 171, dtype=torch.int64))
    tr._save_checkpoint(1, save_best=True)
    for kind in ("latest", "best"):
        for name in ("G", "mpd", "msd"):
            assert os.path.exists(os.path.join(tr.log_dir, f"checkpoint-{kind}-{name}.pth")), (kind, name)
    _, tr2 = make_trainer("cpu", output=tmp_path, resume=tr.log_dir)
    for (k, a), (_, b) in zip(tr.models["msd"].state_dict().items(), tr2.models["msd"].state_dict().items()):
        assert torch.equal(a, b), k
    st1, st2 = tr.optimizer_D.state_dict()["state"], tr2.optimizer_D.state_dict()["state"]
    assert st1.keys() == st2.keys() and len(st1) > 0
    for i in st1:
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st1[i][name], st2[i][name]), (i, name)
    assert tr2.start_epoch == 2


def test_enable_graphs_with_msd_raises():
    _, tr = make_trainer("cpu")
    with pytest.raises(NotImplementedError, match="MSD"):
        tr.enable_graphs(None)


@pytest.mark.parametrize("flag, want", [
    ("ONLY_FEATURE_LOSS", ["multi_resolution_stft", "features_mpd", "features_msd"]),
    ("ONLY_ADVERSARIAL_LOSS", ["multi_resolution_stft", "adversarial_mpd", "adversarial_msd"])])
def test_generator_loss_keys_honour_the_only_flags_cpu(flag, want):
    """trainer/trainer.py:401-426: ONLY_FEATURE_LOSS drops adversarial_msd, ONLY_ADVERSARIAL_LOSS drops features_msd (as for the MPD);
    the kept MSD term has the value it has with both (trainstep_msd.npz), the discriminator's own loss is not touched."""
    from oracle.torch_backend import oracle_stft_patch
    with oracle_stft_patch():
        z, tr = make_trainer("cpu", adversarial={flag: True})
        wave_target = torch.from_numpy(z["wave_target"])
        _, logs = tr._forward_backward(wave_target, wave_target, torch.full((2,), 171, dtype=torch.int64))
    assert [k[len("generator/"):] for k in logs if k.startswith("generator/")] == want
    kept = want[2]
    assert abs(float(logs["generator/" + kept]) - float(z["g::" + kept])) <= 1e-4 * max(1.0, abs(float(z["g::" + kept])))
    total_d = float(z["d::mpd"]) + float(z["d::msd"])
    assert abs(float(logs["total_disc_loss"]) - total_d) <= 1e-4 * max(1.0, abs(total_d))


def test_main_trains_eagerly_when_msd_is_listed_cpu(tmp_path, capsys):
    """main.py's graphs default is off for a yaml that lists "msd" (its next line would otherwise be enable_graphs' NotImplementedError),
    stays on without it, and the tail of main's training path (build_optimizer(capturable=graphs), Trainer, enable_graphs if graphs,
    a step) runs one step with the predicate's answer."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    import main
    yml = os.path.join(GOLDEN, "configs", "vm_asr_48k_MPD.yaml")
    base = ["--cfg", yml, "--output", str(tmp_path)]
    lists = lambda d: ["--opts", "TRAIN.ADVERSARIAL.DISCRIMINATORS", d]      # noqa: E731
    assert main.use_graphs(*main.parse_option(base)) is True
    assert main.use_graphs(*main.parse_option(base + ["--no-graphs"])) is False
    assert main.use_graphs(*main.parse_option(base + ["--accumulation-steps", "2"])) is False
    assert main.use_graphs(*main.parse_option(base + lists("['msd']"))) is False
    args, config = main.parse_option(base + lists("['mpd','msd']"))
    assert config.TRAIN.ADVERSARIAL.DISCRIMINATORS == ["mpd", "msd"] and not args.no_graphs
    graphs = main.use_graphs(args, config)
    assert graphs is False
    woGAN = main.parse_option(["--cfg", os.path.join(GOLDEN, "configs", "vm_asr_16k_woGAN.yaml"), "--output", str(tmp_path)] + lists("['msd']"))
    assert main.use_graphs(*woGAN) is True                      # no adversary is built: nothing of the MSD runs
    from oracle.torch_backend import oracle_stft_patch
    with oracle_stft_patch():
        z, tr = make_trainer("cpu", config.TRAIN.ADVERSARIAL.DISCRIMINATORS, capturable=graphs)
        assert not any(g.get("capturable") for o in (tr.optimizer_G, tr.optimizer_D) for g in o.param_groups)
        before = {k: v.detach().clone() for k, v in tr.models["msd"].named_parameters()}
        wave_target = torch.from_numpy(z["wave_target"])
        if graphs:
            tr.enable_graphs((wave_target, wave_target, torch.full((2,), 171, dtype=torch.int64)))
        _, logs = tr.train_step(wave_target, wave_target, torch.full((2,), 171, dtype=torch.int64))
    assert all(np.isfinite(float(v)) for v in logs.values()) and "generator/features_msd" in logs
    assert all(not torch.equal(v, before[k]) for k, v in tr.models["msd"].named_parameters())


def test_msd_conv_switch_is_declared(monkeypatch):
    """tests/test_knobs.py holds the switches that predate it to a fixed table; this one is checked here: default, values, bad value."""
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_MSD_CONV"]
    assert k.default == "hip" and k.values == ("hip", "torch") and k.kind == "choice" and k.reader == "python:msd"
    monkeypatch.delenv("VMASR_MSD_CONV", raising=False)
    assert knobs.get("VMASR_MSD_CONV") == "hip"
    for v in k.values:
        monkeypatch.setenv("VMASR_MSD_CONV", v)
        assert knobs.get("VMASR_MSD_CONV") == v
    monkeypatch.setenv("VMASR_MSD_CONV", "miopen")
    with pytest.raises(ValueError, match="VMASR_MSD_CONV"):
        knobs.get("VMASR_MSD_CONV")


def test_gconv1d_abi_rejects_bad_arguments():
    """Null pointers and unsupported shapes: the C ABI's invalid-argument code (-1) before anything is launched; the query and its launch-time sibling."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    q, ql = lib.vmasr_gconv1d_supported, lib.vmasr_gconv1d_supported_launch
    for ci, co, g in ((32, 32, 4), (8, 16, 16), (16, 32, 16), (32, 64, 16), (64, 64, 16), (4, 4, 4), (1, 2, 16), (2, 4, 16), (4, 8, 16), (8, 8, 16)):
        assert q(ci * g, co * g, g, 41, 4) == 1
        assert all(ql(ci * g, co * g, g, 41, 4, 20, 2, L) == 1 for L in (1, 2, 5, 19, 1201, 122640))
    assert q(100, 128, 16, 41, 4) == 0 and q(128, 100, 16, 41, 4) == 0 and q(128, 128, 4, 5, 4) == 0 and q(128, 128, 4, 41, 3) == 0
    assert q(128, 128, 0, 41, 4) == 0
    assert ql(128, 128, 4, 41, 4, 41, 2, 100) == 0 and ql(128, 128, 4, 41, 4, 20, 0, 100) == 0 and ql(128, 128, 4, 41, 4, 20, 70000, 100) == 0
    assert ql(128, 128, 4, 41, 4, 0, 2, 40) == 0 and ql(128, 128, 4, 41, 4, 0, 2, 41) == 1           # no output position
    # L = 2^28 gives T = 2^26 outputs = 2^20 weight-gradient units per clip: B * units <= 2^30 (the kernel counts them in 32-bit)
    assert ql(128, 128, 4, 41, 4, 20, 1024, 1 << 28) == 1 and ql(128, 128, 4, 41, 4, 20, 1025, 1 << 28) == 0
    assert lib.vmasr_gconv1d_wgrad_workspace(128, 128, 4, 41, 4, 20, 1025, 1 << 28) == 0
    assert ql(128, 128, 4, 41, 4, 20, 65535, 1 << 20) == 1 and ql(128, 128, 4, 41, 4, 20, 65535, 1 << 23) == 0
    assert lib.vmasr_gconv1d_wgrad_workspace(128, 128, 4, 41, 4, 20, 2, 1201) > 0
    assert lib.vmasr_gconv1d_wgrad_workspace(100, 128, 16, 41, 4, 20, 2, 1201) == 0
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused first
    assert lib.vmasr_gconv1d_fwd(None, p, p, p, p, 2, 128, 128, 4, 100, 41, 4, 20, 1, None) == -1
    assert b"null" in lib.vmasr_last_error()
    assert lib.vmasr_gconv1d_fwd(p, p, p, p, None, 2, 128, 128, 4, 100, 41, 4, 20, 1, None) == -1      # the activation needs pre
    assert lib.vmasr_gconv1d_fwd(p, p, p, p, p, 2, 100, 128, 16, 100, 41, 4, 20, 1, None) == -1
    assert b"unsupported shape" in lib.vmasr_last_error()
    assert lib.vmasr_gconv1d_dgrad(p, p, None, p, 2, 128, 128, 4, 100, 41, 4, 20, None) == -1
    assert lib.vmasr_gconv1d_dgrad(p, p, p, p, 2, 128, 128, 4, 100, 5, 4, 20, None) == -1
    assert lib.vmasr_gconv1d_wgrad(p, p, p, None, None, p, 1 << 30, 2, 128, 128, 4, 100, 41, 4, 20, None) == -1
    assert lib.vmasr_gconv1d_wgrad(p, p, p, p, p, p, 16, 2, 128, 128, 4, 100, 41, 4, 20, None) == -1
    assert b"workspace" in lib.vmasr_last_error()
    assert lib.vmasr_gconv1d_wgrad(p, p, p, p, p, p, 1 << 30, 2, 128, 128, 3, 100, 41, 4, 20, None) == -1
