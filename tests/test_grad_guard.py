"""The gradient guard on the CPU (no HIP path there: grad_guard.GradGuard forms its four values with torch): the trainer's
optimizer.step() route — skip of a non-finite step, clipping by global norm —, the defaults, and the CLI flags."""
import copy

import pytest
import torch

from test_trainer import _batch, _tiny_config


def _trainer(cfg, **kw):
    import vm_asr_amd
    from oracle.torch_backend import use_oracle
    from vm_asr_amd.trainer import Trainer, build_optimizer
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    use_oracle(models["generator"])
    opts = {"generator": build_optimizer(cfg, models["generator"]), "discriminator": build_optimizer(cfg, [models["mpd"]])}
    tr = Trainer(models, [], opts, cfg, torch.device("cpu"), None, None, {}, amp=False, gan=True, len_epoch=0, **kw)
    for m in tr.models.values():
        m.train()
    return tr


def _trained_state(tr):
    """Clones of every parameter and every optimiser state tensor (what a skipped step must leave alone)."""
    out = [p.detach().clone() for k in ("generator", "mpd") for p in tr.models[k].parameters()]
    for o in (tr.optimizer_G, tr.optimizer_D):
        for g in o.param_groups:
            for p in g["params"]:
                out += [v.detach().clone() for v in o.state.get(p, {}).values() if torch.is_tensor(v)]
    return out


def _copy_into(dst, src):
    """dst continues from src's state: weights, buffers (spectral-norm u / v) and optimiser states."""
    for k in ("generator", "mpd"):
        dst.models[k].load_state_dict(src.models[k].state_dict())
    dst.optimizer_G.load_state_dict(copy.deepcopy(src.optimizer_G.state_dict()))
    dst.optimizer_D.load_state_dict(copy.deepcopy(src.optimizer_D.state_dict()))
    dst.global_step = src.global_step


def test_cpu_trainer_skips_a_nonfinite_step_and_clips_by_global_norm():
    from oracle.torch_backend import oracle_stft_patch
    cfg = _tiny_config()
    batches = [_batch(cfg, 2, seed=s) for s in range(4)]
    guarded, plain = _trainer(cfg, skip_nonfinite=True), _trainer(cfg)
    assert len(guarded.grad_guards) == 2 and plain.grad_guards is None
    with oracle_stft_patch():
        guarded.train_step(*batches[0])                        # creates the optimiser states
        clean = guarded.guard_report()
        assert clean["skipped_G"] == clean["skipped_D"] == 0 and clean["grad_norm_G"] > 0 and clean["grad_norm_D"] > 0
        # ---- one poisoned step: a tensor hook turns one parameter's gradient into inf / NaN
        # (one in each model: there is one guard per optimiser, and a clean optimiser steps on while the other one skips)
        victims = [next(p for n, p in guarded.models[k].named_parameters() if n.endswith("bias") and p.requires_grad)
                   for k in ("generator", "mpd")]
        hooks = [v.register_hook(lambda g: g * float("inf")) for v in victims]
        before = _trained_state(guarded)
        guarded.train_step(*batches[1])
        for h in hooks:
            h.remove()
        after = _trained_state(guarded)
        assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
        rep = guarded.grad_guards[0].read()
        assert rep["skipped"] == 1 and rep["found_inf"] and guarded.grad_guards[1].read()["skipped"] == 1
        # ---- the next, clean step == the step of an unguarded trainer started from the same state
        _copy_into(plain, guarded)
        guarded.train_step(*batches[2])
        plain.train_step(*batches[2])
        for k in ("generator", "mpd"):
            for (n, a), (_, b) in zip(guarded.models[k].named_parameters(), plain.models[k].named_parameters()):
                assert torch.equal(a, b), (k, n)
        assert guarded.grad_guards[0].read()["skipped"] == 1 and not guarded.grad_guards[0].read()["found_inf"]
        # ---- clip_grad below the measured norms == an unguarded step preceded by clip_grad_norm_
        norms = guarded.guard_report()
        max_norm = 0.5 * min(norms["grad_norm_G"], norms["grad_norm_D"])
        clipped = _trainer(cfg, clip_grad=max_norm)
        _copy_into(clipped, guarded)
        _copy_into(plain, guarded)
        plain_steps = plain._optimizer_steps

        def clip_then_step():
            for o in (plain.optimizer_G, plain.optimizer_D):
                torch.nn.utils.clip_grad_norm_([p for g in o.param_groups for p in g["params"]], max_norm)
            plain_steps()
        plain._optimizer_steps = clip_then_step
        clipped.train_step(*batches[3])
        plain.train_step(*batches[3])
        for guard in clipped.grad_guards:
            r = guard.read()
            assert r["grad_norm"] > max_norm and abs(r["clip_coef"] - max_norm / (r["grad_norm"] + 1e-6)) <= 1e-6 * r["clip_coef"]
        moved = 0
        for k in ("generator", "mpd"):
            for (n, a), (_, b), (_, c) in zip(clipped.models[k].named_parameters(), plain.models[k].named_parameters(),
                                              guarded.models[k].named_parameters()):
                assert torch.allclose(a, b, rtol=0, atol=1e-7 * max(1.0, float(b.detach().abs().max()))), (k, n)
                moved += int(not torch.equal(a, c))
        assert moved > 100


class _Lines:
    def __init__(self):
        self.lines = []

    def info(self, m):
        self.lines.append(m)

    warning = info


def test_defaults_build_no_guard_and_an_uncapturable_guard_stays_eager(monkeypatch):
    cfg = _tiny_config()
    tr = _trainer(cfg)
    assert tr.grad_guards is None and tr._grad_guards() is None and tr.guard_report() == {}
    assert tr.skip_nonfinite is False and tr.clip_grad is None
    with pytest.raises(ValueError):
        _trainer(cfg, clip_grad=0.0)
    # guard on, the HIP AdamW route switched off: enable_graphs() must not capture a host read — one log line, eager
    monkeypatch.setenv("VMASR_HIP_ADAMW", "0")
    tr = _trainer(cfg, skip_nonfinite=True)
    tr.logger = _Lines()
    assert tr.enable_graphs(_batch(cfg, 2)) is False
    assert tr._graphed is None and len(tr.logger.lines) == 1 and "gradient guard" in tr.logger.lines[0] and "eager" in tr.logger.lines[0]


def test_cli_shows_both_flags(capsys):
    import main
    with pytest.raises(SystemExit):
        main.parse_option(["--help"])
    text = capsys.readouterr().out
    assert "--skip-nonfinite" in text and "--clip-grad FLOAT" in text


def test_cpu_guard_values_and_counter():
    from vm_asr_amd.grad_guard import GradGuard
    torch.manual_seed(0)
    gs = [torch.randn(5, 3), torch.randn(7)]
    g = GradGuard(gs, "cpu", max_norm=0.5)
    g.measure()
    want = torch.sqrt(sum((t.double() ** 2).sum() for t in gs)).item()
    r = g.read()
    assert abs(r["grad_norm"] - want) <= 1e-6 * want and abs(r["clip_coef"] - 0.5 / (want + 1e-6)) <= 1e-6 and not r["found_inf"]
    gs[1][3] = float("nan")
    g.measure(); g.measure()
    assert g.read()["found_inf"] and g.read()["skipped"] == 2 and g.still_valid()
    gs[1][3] = 1e30                                   # finite elements, overflowing squares: not a non-finite gradient
    g.measure()
    r = g.read()
    assert not r["found_inf"] and r["skipped"] == 2 and float(g.state[4]) == 1.0
    assert abs(r["grad_norm"] - 1e30) <= 1e-6 * 1e30 and abs(r["clip_coef"] - 0.5 / r["grad_norm"]) <= 1e-6 * r["clip_coef"]
    assert GradGuard(gs, "cpu").max_norm == 0.0
