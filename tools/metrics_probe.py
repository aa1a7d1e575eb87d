"""What the fused metrics operator costs, measured on the GPU (writes a Markdown report, profiles/metrics_fused.md):

  (a) device time of one evaluation at B = 4, T = 122 640: metric.per_clip against the four composed functions as
      Trainer._metrics calls them, without their float() reads — HIP events around windows of calls, the two alternated;
  (b) ms per train step of the flagship workload (vm_asr_48k_MPD, batch 4, graphs on) with no metrics, with the composed metrics
      read on the host every step (what bench.py --with-metrics times), and with metric.Accumulator.update every step and one
      read at the end — the three legs alternated over several rounds on ONE trainer, host clock around synchronised windows.

    python tools/metrics_probe.py --out profiles/metrics_fused.md
"""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # vm_asr_amd/hip_env.py: before the GPU is initialised
os.environ.setdefault("TENSILE_STREAMK_DATA_PARALLEL", "1")

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(fn, calls):
    """device ms per call of `fn` over a window of `calls` back-to-back calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def evaluation_time(device, calls, rounds):
    from vm_asr_amd import metric
    g = torch.Generator().manual_seed(9)
    tgt = (0.1 * torch.randn(4, 122640, generator=g)).to(device)
    out = tgt + (0.03 * torch.randn(4, 122640, generator=g)).to(device)
    hf = torch.tensor([171, 342, 513, 1024], device=device)
    mets = [metric.snr, metric.lsd, metric.lsd_hf, metric.lsd_lf]

    def composed():
        return [m(out, tgt, hf=hf) for m in mets]      # (lsd_hf / lsd_lf read hf on the host: part of the composed path)

    def fused():
        return metric.per_clip(out, tgt, hf)
    for _ in range(5):
        composed()
        fused()
    torch.cuda.synchronize()
    ms = {"composed": [], "fused": []}
    for _ in range(rounds):
        ms["composed"].append(_event_ms(composed, calls))
        ms["fused"].append(_event_ms(fused, calls))
    agree = [abs(float(a) - float(b)) for a, b in zip(composed(), fused().double().mean(0))]
    return ms, agree


def step_cost(device, steps, rounds):
    import bench
    from vm_asr_amd import metric
    from vm_asr_amd.trainer import default_metric_ftns
    config = bench.make_config("vm_asr_48k_MPD", 4)
    trainer = bench.build_trainer(config, device, amp=True, capturable=True)
    for m in trainer.models.values():
        m.train()
    batch = bench.synth_batch(config, device, 0)
    if not trainer.enable_graphs(batch, warmup=3):
        raise SystemExit(f"HIP graph capture failed: {getattr(trainer, 'graph_error', None)}")
    mets = default_metric_ftns(config)
    acc = metric.Accumulator(device)

    def none():
        trainer.train_step(*batch)

    def composed():
        res = trainer.train_step(*batch)
        for m in mets:
            float(m(res[0].float().squeeze(1), batch[1].squeeze(1), hf=batch[2]))

    def accumulated():
        res = trainer.train_step(*batch)
        acc.update(res[0], batch[1], batch[2])
    legs = {"none": none, "composed": composed, "accumulator": accumulated}
    for fn in legs.values():
        for _ in range(3):
            fn()
    acc.read()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            if name == "accumulator":
                acc.read()                      # the one host read, inside the window
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    return ms


def _fmt(vals):
    return f"{statistics.median(vals):.3f} (min {min(vals):.3f}, max {max(vals):.3f}, {len(vals)} windows)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--calls", type=int, default=50, help="(a) calls per event-timed window")
    ap.add_argument("--steps", type=int, default=20, help="(b) train steps per window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip (b)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_probe.py measures on the GPU"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lines = ["# Fused SNR / LSD / LSD-HF / LSD-LF operator: cost on the GPU", "",
             f"`python tools/metrics_probe.py` on {torch.cuda.get_device_properties(device).name}, torch {torch.__version__}.", ""]
    ev, agree = evaluation_time(device, args.calls, args.rounds)
    c, f = statistics.median(ev["composed"]), statistics.median(ev["fused"])
    lines += ["## (a) device time per evaluation, B = 4, T = 122 640", "",
              f"HIP events around windows of {args.calls} calls, composed and fused alternated, median over windows (ms per evaluation).", "",
              "| path | ms per evaluation |", "|---|---|",
              f"| composed: snr, lsd, lsd_hf, lsd_lf as `Trainer._metrics` calls them, no `float()` | {_fmt(ev['composed'])} |",
              f"| fused: `metric.per_clip` | {_fmt(ev['fused'])} |", "",
              f"fused / composed = {f / c:.3f} (requirement: <= 0.5: {'met' if f <= 0.5 * c else 'MISSED'}).  "
              f"|composed - fused| of the batch means (snr, lsd, lsd_hf, lsd_lf): " + ", ".join(f"{v:.2e}" for v in agree) + ".", ""]
    if not args.no_step:
        st = step_cost(device, args.steps, args.rounds)
        n, cm, am = (statistics.median(st[k]) for k in ("none", "composed", "accumulator"))
        lines += ["## (b) train step, vm_asr_48k_MPD, batch 4, bf16 autocast, graphs on", "",
                  f"Host clock around synchronised windows of {args.steps} steps, the three legs alternated on one trainer, median over windows.", "",
                  "| leg | ms per step | over no metrics |", "|---|---|---|",
                  f"| no metrics | {_fmt(st['none'])} | |",
                  f"| composed metrics, read every step | {_fmt(st['composed'])} | {cm - n:+.3f} ms = {100 * (cm - n) / n:+.2f} % |",
                  f"| `Accumulator.update` every step, one read per window | {_fmt(st['accumulator'])} | {am - n:+.3f} ms = {100 * (am - n) / n:+.2f} % |", "",
                  f"Accumulator overhead smaller than the composed path's: {'yes' if am - n < cm - n else 'NO'}.  "
                  f"Against the 1 % of a step the per-step metrics are allowed: {100 * (am - n) / n:+.2f} %.", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
