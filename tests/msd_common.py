"""Shared by tests/test_msd.py (CPU) and tests/test_msd_gpu.py: fixture loading and the comparisons against tests/golden/msd.npz /
trainstep_msd.npz (made from the reference by tests/golden/make_msd_golden.py)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from msd_weights import state_dict_from  # noqa: E402

N_DISC, N_FMAP = 3, 8
GRAD_NAMES = ["discriminators.0.convs.1.parametrizations.weight.original", "discriminators.1.convs.3.parametrizations.weight.original",
              "discriminators.2.conv_post.bias"]


def fixture_state(z, prefix=""):
    """(keys, shapes, state_dict of torch tensors) stored under `prefix`."""
    keys = [str(k) for k in z[prefix + "keys"]]
    shapes = {k: tuple(int(d) for d in str(s).split(",") if d) for k, s in zip(keys, z[prefix + "shapes"])}
    sd = {k: torch.from_numpy(v) for k, v in state_dict_from(z, prefix, shapes).items()}
    return keys, shapes, {k: sd[k] for k in keys}


def close(got, want, tol, what):
    """max|got - want| <= tol * max|want| (the form of tests/test_mpd.py::_close), reported to the parity table."""
    import errtable
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(np.abs(want).max(), 1e-6)
    err = np.abs(got - want).max()
    errtable.record(what, got, want, tol * scale)
    print(f"{what}: err {err:.3e} scale {scale:.3e} allowed {tol * scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def load_msd(device):
    from vm_asr_amd.msd import MultiScaleDiscriminator
    z = np.load(os.path.join(GOLDEN, "msd.npz"))
    D = MultiScaleDiscriminator(hidden=16)
    _, _, sd = fixture_state(z)
    D.load_state_dict(sd, strict=True)
    return z, D.to(device)


def run_eval(device, tol):
    """Eval-mode scores, feature maps, the three losses and the three gradients against the golden; then one train-mode forward: u, v."""
    from vm_asr_amd.loss import HiFiGANLoss
    z, D = load_msd(device)
    D.eval()
    y, y_hat = torch.from_numpy(z["y"]).to(device), torch.from_numpy(z["y_hat"]).to(device)
    L = HiFiGANLoss("lsgan")
    rs, gs, fr, fg = D(y, y_hat)
    for i in range(N_DISC):
        close(rs[i], z[f"eval_real{i}"], tol, f"real{i}")
        close(gs[i], z[f"eval_gen{i}"], tol, f"gen{i}")
        assert len(fr[i]) == N_FMAP and len(fg[i]) == N_FMAP
        for j in range(N_FMAP):
            close(fr[i][j], z[f"eval_fmap_real{i}_{j}"], tol, f"fmap_real{i}_{j}")
            close(fg[i][j], z[f"eval_fmap_gen{i}_{j}"], tol, f"fmap_gen{i}_{j}")
    d_loss, g_loss, f_loss = L.discriminator_loss(rs, gs), L.generator_loss(gs), L.feature_loss(fr, fg)
    for name, v in (("d_loss", d_loss), ("g_loss", g_loss), ("f_loss", f_loss)):
        assert abs(v.item() - float(z[name])) <= tol * max(1.0, abs(float(z[name]))), (name, v.item(), float(z[name]))
    d_loss.backward()
    params = dict(D.named_parameters())
    for n in GRAD_NAMES:
        close(params[n].grad, z[f"d_disc::{n}"], 5 * tol, n)
    D.train()
    with torch.no_grad():
        D(y, y_hat)
    sd, n = D.state_dict(), 0
    for k in z.files:
        if k.startswith("train_after::"):
            close(sd[k[13:]], z[k], tol, k)
            n += 1
    assert n == 48      # 24 spectrally normalised weights x (u, v)
    return z, D


class LeafGenerator(nn.Module):
    """Stands in for the generator: a fixed `wave_out` that is a leaf requiring grad (tests/test_trainstep.py)."""

    def __init__(self, wave):
        super().__init__()
        self.wave = nn.Parameter(wave.clone())

    def forward(self, x, hf):
        return self.wave * 1.0


def make_trainer(device, discriminators=("mpd", "msd"), output=None, resume=None, adversarial=None, capturable=None):
    """adversarial: overrides of TRAIN.ADVERSARIAL fields; capturable: not None -> the optimisers come from trainer.build_optimizer, as main.py's do."""
    from vm_asr_amd.config import get_default_config, update_config
    from vm_asr_amd.discriminator import MultiPeriodDiscriminator
    from vm_asr_amd.msd import MultiScaleDiscriminator
    from vm_asr_amd.trainer import Trainer
    z = np.load(os.path.join(GOLDEN, "trainstep_msd.npz"))
    c = get_default_config()
    c.TRAIN.ADVERSARIAL.ENABLE = True
    c.TRAIN.ADVERSARIAL.DISCRIMINATORS = list(discriminators)
    c.TRAIN.ADVERSARIAL.MPD_HIDDEN = 2
    for k, v in (adversarial or {}).items():
        assert hasattr(c.TRAIN.ADVERSARIAL, k), k
        setattr(c.TRAIN.ADVERSARIAL, k, v)
    if output is not None:
        c.OUTPUT = str(output)
    if resume is not None:
        c.MODEL.RESUME_PATH = str(resume)
    cfg = update_config(c)
    models = {"generator": LeafGenerator(torch.from_numpy(z["wave_out"]))}
    if "mpd" in discriminators:
        models["mpd"] = MultiPeriodDiscriminator(hidden=2)
        if resume is None:
            models["mpd"].load_state_dict(fixture_state(z, "mpd_")[2], strict=True)
    if "msd" in discriminators:
        models["msd"] = MultiScaleDiscriminator(hidden=16)
        if resume is None:
            models["msd"].load_state_dict(fixture_state(z, "msd_")[2], strict=True)
    d_params = [p for k in discriminators for p in models[k].parameters()]
    if capturable is None:
        opts = {"generator": torch.optim.AdamW(models["generator"].parameters(), lr=1e-4), "discriminator": torch.optim.AdamW(d_params, lr=1e-4)}
    else:
        from vm_asr_amd.trainer import build_optimizer
        opts = {"generator": build_optimizer(cfg, models["generator"], capturable=capturable),
                "discriminator": build_optimizer(cfg, [models[d] for d in cfg.TRAIN.ADVERSARIAL.DISCRIMINATORS], capturable=capturable)}
    tr = Trainer(models, [], opts, cfg, torch.device(device), None, None, {}, amp=False, gan=True, len_epoch=0, dp_mode="flat")
    for m in tr.models.values():
        m.train()
    return z, tr


# loss values 1e-4, gradients 3e-4 in relative L2 and 2e-3 of the peak: the bounds tests/test_trainstep.py holds the converged ("warm")
# MPD step to, for the reasons written there (the MPD's four power iterations run up front; L1-type losses flip signs at near-ties).
# The MSD follows the reference's schedule pass by pass, so it needs no allowance of its own.
TOL_VAL, TOL_GRAD, TOL_MAX = 1e-4, 3e-4, 2e-3


def check_trainstep(device):
    """One evaluation of the trainer's losses + both backward passes for ["mpd", "msd"] against trainstep_msd.npz."""
    from vm_asr_amd.trainer import unwrap
    z, tr = make_trainer(device)
    wave_target = torch.from_numpy(z["wave_target"]).to(device)
    hf = torch.full((wave_target.shape[0],), 171, dtype=torch.int64, device=device)
    _, logs = tr._forward_backward(wave_target, wave_target, hf)
    g_keys = [k[len("generator/"):] for k in logs if k.startswith("generator/")]
    assert g_keys == [str(k) for k in z["g_keys"]] == ["multi_resolution_stft", "adversarial_mpd", "features_mpd", "adversarial_msd", "features_msd"]
    for k in g_keys:
        w = float(z[f"g::{k}"])
        print(f"generator/{k}: got {float(logs['generator/' + k]):.6f} want {w:.6f}")
        assert abs(float(logs[f"generator/{k}"]) - w) <= TOL_VAL * max(1.0, abs(w)), (k, float(logs[f"generator/{k}"]), w)
    total_g = sum(float(z[f"g::{k}"]) for k in g_keys)
    total_d = sum(float(z[f"d::{k}"]) for k in z["d_keys"])
    assert [str(k) for k in z["d_keys"]] == ["mpd", "msd"]
    assert abs(float(logs["total_loss"]) - total_g) <= TOL_VAL * max(1.0, abs(total_g))
    assert abs(float(logs["total_disc_loss"]) - total_d) <= TOL_VAL * max(1.0, abs(total_d)), (float(logs["total_disc_loss"]), total_d)

    def close2(got, ref, what):
        got = got.detach().double().cpu().numpy()
        assert got.shape == ref.shape, what
        err, scale = np.abs(got - ref).max(), max(np.abs(ref).max(), 1e-12)
        rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
        print(f"{what}: max err {err:.3e} of {scale:.3e}, rel L2 {rel:.3e}")
        assert err <= TOL_MAX * scale and rel <= TOL_GRAD, (what, err, scale, rel)
    close2(tr.models["generator"].wave.grad, z["dwave"], "d total_g / d wave_out")
    msd = unwrap(tr.models["msd"])
    params = dict(msd.named_parameters())
    for n in GRAD_NAMES:
        close2(params[n].grad, z[f"dD::{n}"], n)
    sd = msd.state_dict()
    for k in z.files:
        if k.startswith("msd_after::"):
            close2(sd[k[11:]], z[k], k)
    return z, tr
