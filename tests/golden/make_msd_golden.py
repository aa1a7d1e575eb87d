"""Golden fixtures of the multi-scale discriminator, made from the REFERENCE on the build machine (tests/golden/_refload.py loads it
from where it lies; nothing of it is copied):

  msd.npz            model/discriminator.py:174-313, MultiScaleDiscriminator(hidden=16) on a 2 x 1 x 1201 pair: the state_dict, eval-mode
                     scores and all 24 + 24 feature maps, the LSGAN discriminator / generator / feature losses (model/loss.py:188-235),
                     d(discriminator loss) / d(three weights), and u / v after one train-mode forward(y, y_hat).
                     hidden 16 is the smallest width the group counts divide; the lengths run 1201 -> 301 -> 76 -> 19 -> 5 -> 2 through
                     scale 1 and 601 / 301 into scales 2 and 3: windows shorter than the kernel, lengths that the stride does not divide.
  trainstep_msd.npz  trainer/trainer.py:318-426 (`_get_losses`, `_get_mpd_loss`, `_get_msd_loss`, `_get_stft_loss`, taken by AST as
                     make_golden.py::gen_trainstep does) with DISCRIMINATORS = ["mpd", "msd"], MPD hidden 2 (u, v converged: the
                     trainer's MPD schedule differs from the reference's while they move, tests/test_trainstep.py) and MSD hidden 16:
                     every loss value, the three MSD gradients of the discriminator loss, MSD u / v after the step.

The weights with >= 1024 elements are not stored but seeded (msd_weights.py); they are written into the reference module first.

    python tests/golden/make_msd_golden.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refload import REF, load_reference  # noqa: E402
from msd_weights import MIN_SEEDED, seeded  # noqa: E402

GRAD_NAMES = ["discriminators.0.convs.1.parametrizations.weight.original",      # groups 4
              "discriminators.1.convs.3.parametrizations.weight.original",      # groups 16
              "discriminators.2.conv_post.bias"]


def _np(t):
    return t.detach().cpu().numpy().copy()       # (a copy: state_dict tensors are live, later forwards move u / v in place)


def _seed_weights(D, first_seed):
    """Overwrite the large tensors of D's state with seeded values (seeds first_seed, first_seed + 1, ... in state_dict order)."""
    seed = first_seed
    with torch.no_grad():
        for v in D.state_dict().values():
            if v.numel() >= MIN_SEEDED:
                v.copy_(torch.from_numpy(seeded(seed, tuple(v.shape))))
                seed += 1


def _record_state(D, out, prefix, first_seed):
    """D's state under `prefix`: small tensors stored, the seeded ones as their seed (checked against the module's values)."""
    sd = D.state_dict()
    seed = first_seed
    for k, v in sd.items():
        if v.numel() >= MIN_SEEDED:
            assert np.array_equal(_np(v), seeded(seed, tuple(v.shape))), k
            out[f"{prefix}seed::{k}"] = np.array([seed], dtype=np.int64)
            seed += 1
        else:
            out[f"{prefix}sd::{k}"] = _np(v)
    out[f"{prefix}keys"] = np.array(list(sd.keys()))
    out[f"{prefix}shapes"] = np.array([",".join(str(int(d)) for d in v.shape) for v in sd.values()])


def gen_msd(ns):
    torch.manual_seed(31)
    D = ns.discriminator.MultiScaleDiscriminator(hidden=16)
    out = {}
    _seed_weights(D, 1000)
    g = torch.Generator().manual_seed(32)
    y = 0.3 * torch.randn(2, 1, 1201, generator=g)
    y_hat = 0.3 * torch.randn(2, 1, 1201, generator=g)
    D.train()
    with torch.no_grad():
        for _ in range(10):            # u, v follow the seeded weights (20 power iterations) before anything is recorded
            D(y, y_hat)
    _record_state(D, out, "", 1000)
    out.update(y=_np(y), y_hat=_np(y_hat))
    L = ns.loss.HiFiGANLoss("lsgan")
    D.eval()
    rs, gs, fr, fg = D(y, y_hat)
    for i, (a, b) in enumerate(zip(rs, gs)):
        out[f"eval_real{i}"], out[f"eval_gen{i}"] = _np(a), _np(b)
    for i, (a, b) in enumerate(zip(fr, fg)):
        for j, (u, v) in enumerate(zip(a, b)):
            out[f"eval_fmap_real{i}_{j}"], out[f"eval_fmap_gen{i}_{j}"] = _np(u), _np(v)
    d_loss, g_loss, f_loss = L.discriminator_loss(rs, gs), L.generator_loss(gs), L.feature_loss(fr, fg)
    out.update(d_loss=np.array(d_loss.item()), g_loss=np.array(g_loss.item()), f_loss=np.array(f_loss.item()))
    params = dict(D.named_parameters())
    d_loss.backward()
    for n in GRAD_NAMES:
        out[f"d_disc::{n}"] = _np(params[n].grad)
    D.train()
    with torch.no_grad():
        D(y, y_hat)
    for k, v in D.state_dict().items():
        if k.endswith("._u") or k.endswith("._v"):
            out[f"train_after::{k}"] = _np(v)
    print(f"  msd: d={d_loss.item():.5f} g={g_loss.item():.5f} f={f_loss.item():.5f}")
    np.savez_compressed(os.path.join(HERE, "msd.npz"), **out)


def gen_trainstep_msd(ns):
    src = open(os.path.join(REF, "trainer/trainer.py")).read()
    cls = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Trainer"][0]
    want = ("_get_losses", "_get_mpd_loss", "_get_msd_loss", "_get_stft_loss")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == 4
    g = dict(torch=torch, mae_loss=ns.loss.mae_loss, mse_loss=ns.loss.mse_loss)
    exec(compile(ast.Module(body=fns, type_ignores=[]), "reference_trainer_losses", "exec"), g)
    NS = types.SimpleNamespace
    cfg = NS(TRAIN=NS(LOSSES=NS(GEN=["multi_resolution_stft"]),
                      ADVERSARIAL=NS(DISCRIMINATORS=["mpd", "msd"], ONLY_FEATURE_LOSS=False, ONLY_ADVERSARIAL_LOSS=False,
                                     FEATURE_LOSS_LAMBDA=100, GAN_LOSS_TYPE="lsgan")))
    gen = torch.Generator().manual_seed(41)
    T = 6000
    wave_target = 0.1 * torch.randn(2, 1, T, generator=gen)
    wave_out0 = wave_target + 0.03 * torch.randn(2, 1, T, generator=gen)
    out = dict(wave_target=_np(wave_target), wave_out=_np(wave_out0))
    torch.manual_seed(42)
    mpd = ns.discriminator.MultiPeriodDiscriminator(hidden=2)
    msd = ns.discriminator.MultiScaleDiscriminator(hidden=16)
    mpd.train()
    msd.train()
    _seed_weights(mpd, 3000)
    _seed_weights(msd, 2000)
    with torch.no_grad():
        for _ in range(1000):          # the MPD's u, v converged (2000 power iterations per weight)
            mpd(wave_target, wave_out0)
        for _ in range(2):             # the MSD's u, v still move: its passes see four different sigmas, as in the first steps of a run
            msd(wave_target, wave_out0)
    _record_state(mpd, out, "mpd_", 3000)
    _record_state(msd, out, "msd_", 2000)
    me = NS(config=cfg, gan=True, models={"mpd": mpd, "msd": msd},
            multi_resolution_stft=ns.loss.MultiResolutionSTFTLoss(factor_sc=0.5, factor_mag=0.5, emphasize_high_freq=False),
            higi_gan_loss=ns.loss.HiFiGANLoss("lsgan"))
    for f in want:
        setattr(me, f, types.MethodType(g[f], me))
    wave_out = wave_out0.clone().requires_grad_()
    losses = me._get_losses(wave_out, wave_target)
    out["g_keys"] = np.array(list(losses["generator"].keys()))
    out["d_keys"] = np.array(list(losses["discriminator"].keys()))
    for k, v in losses["generator"].items():
        out[f"g::{k}"] = np.array(v.item())
    for k, v in losses["discriminator"].items():
        out[f"d::{k}"] = np.array(v.item())
    total_g, total_d = sum(losses["generator"].values()), sum(losses["discriminator"].values())
    total_g.backward(retain_graph=True)
    out["dwave"] = _np(wave_out.grad)
    params = dict(msd.named_parameters())
    for m in (mpd, msd):
        for p in m.parameters():
            p.grad = None                  # optimizer_D.zero_grad() (trainer/trainer.py:435)
    total_d.backward()
    for n in GRAD_NAMES:
        out[f"dD::{n}"] = _np(params[n].grad)
    for k, v in msd.state_dict().items():
        if k.endswith("._u") or k.endswith("._v"):
            out[f"msd_after::{k}"] = _np(v)
    print("  trainstep_msd: " + " ".join(f"{k}={v.item():.5f}" for k, v in {**losses["generator"], **losses["discriminator"]}.items()))
    np.savez_compressed(os.path.join(HERE, "trainstep_msd.npz"), **out)


if __name__ == "__main__":
    ns = load_reference()
    gen_msd(ns)
    gen_trainstep_msd(ns)
