"""Cost of the gradient guard (vm_asr_amd/grad_guard.py, csrc/gradnorm.hip) on the flagship workload, vm_asr_48k_MPD:

  1. measure() over the generator's and the MPD's gradient views (HIP events around windows of 300 calls, several ms each; GB/s at
     4 B per element),
  2. the guarded against the unguarded AdamW launch on the same buffers (28 B per element: the project's streaming yardstick),
  3. the captured training step with the guard off and on, timed in alternating blocks in ONE process, with the spread of the
     off/off repeats beside the on - off difference.

    python tools/bench_grad_guard.py [--batch 4] [--rounds 6] [--steps 10]

Prints one JSON line; profiles/grad_guard.md holds a recorded run.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (sets the runtime environment before torch initialises the GPU)
import torch  # noqa: E402


def timed(fn, calls, reps, warmup=3):
    """Median / min / max microseconds per call of `fn` over `reps` event-bracketed batches of `calls` calls."""
    for _ in range(warmup * calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / calls)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def build(cfg, dev, batch, guard):
    from vm_asr_amd.trainer import Trainer, build_optimizer
    import vm_asr_amd
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    for m in models.values():
        m.to(dev)
    opts = {"generator": build_optimizer(cfg, models["generator"], True), "discriminator": build_optimizer(cfg, [models["mpd"]], True)}
    tr = Trainer(models, [], opts, cfg, dev, None, None, {}, amp=True, gan=True, len_epoch=0, dp_mode="flat", skip_nonfinite=guard)
    for m in tr.models.values():
        m.train()
    tr.train_step(*batch)
    if not tr.enable_graphs(batch, warmup=2):
        raise SystemExit(f"capture failed: {tr.graph_error}")
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("vm_asr_48k_MPD", args.batch)
    batch = bench.synth_batch(cfg, dev, 0)
    from vm_asr_amd.fused_adamw import HipAdamWStep
    on = build(cfg, dev, batch, guard=True)
    res = {"workload": "vm_asr_48k_MPD", "batch": args.batch, "device": torch.cuda.get_device_properties(dev).name}
    shadows = {id(s): d for s, d in zip(on._shadow_params, on._shadow_dst)}
    snap = on._snapshot_training_state()       # the timed AdamW calls below are thousands of real updates on one gradient: undone after
    for name, guard, fused, opt in zip(("generator", "mpd"), on.grad_guards, on._hip_adamw, (on.optimizer_G, on.optimizer_D)):
        assert guard.still_valid() and fused.still_valid()
        plain = HipAdamWStep(opt, shadows, on._shadow_t)
        n = guard.total
        m = timed(guard.measure, 300, 10, warmup=1)
        a0, a1 = timed(plain.step, 200, 10, warmup=1), timed(fused.step, 200, 10, warmup=1)
        res[name] = {"elements": n, "segments": int(guard.segments.numel() // 16), "chunks": guard.nchunks, "measure": m,
                     "measure_GBps": round(4e-3 * n / m["median_us"], 1),
                     "adamw_unguarded": a0, "adamw_unguarded_GBps": round(28e-3 * fused.total / a0["median_us"], 1),
                     "adamw_guarded": a1, "adamw_guarded_GBps": round(28e-3 * fused.total / a1["median_us"], 1)}
    torch.cuda.synchronize()
    on._restore_training_state(snap)
    off = build(cfg, dev, batch, guard=False)
    res["layout_on"], res["layout_off"] = on.graph_variants, off.graph_variants

    def block(tr):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            tr.train_step(*batch)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps
    for tr in (off, on):
        block(tr)
    t_off, t_on = [], []
    for _ in range(args.rounds):            # off, off, on: the off/off pair gives the noise floor of the same comparison
        a, b, c = block(off), block(off), block(on)
        t_off.append((a, b))
        t_on.append(c)
    res["step_ms_off"] = round(statistics.median([x for p in t_off for x in p]), 4)
    res["step_ms_on"] = round(statistics.median(t_on), 4)
    res["on_minus_off_ms"] = [round(c - 0.5 * (a + b), 4) for (a, b), c in zip(t_off, t_on)]
    res["off_minus_off_ms"] = [round(b - a, 4) for a, b in t_off]
    res["skipped"] = [g.read()["skipped"] for g in on.grad_guards]
    assert res["skipped"] == [0, 0], "the timed steps were skipped: the on / off comparison is void"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
