"""Time of the one-launch HIP SGD step (vm_asr_amd/fused_sgd.py, csrc/sgd.hip) on the parameter set of vm_asr_48k_MPD, generator and
period discriminator, each as one optimiser as in training:

  * HipSgdStep without / with bf16 shadows (every parameter, plus the transposed shadow of every 2-D weight) and without / with the
    gradient guard (the guard's own measure() is not in the window: tools/bench_grad_guard.py times it),
  * torch.optim.SGD(foreach=True) and (fused=True) with the same device learning-rate tensor on the same tensors,
  * HipAdamWStep on the same tensors: the project's streaming yardstick (28 B per parameter against SGD's 20).

Gradients are seeded noise in one flat buffer per model, as the trainer lays them out; nothing is trained.  Device events around
windows of `--calls` calls, `--reps` windows after a warm-up, nothing else running; achieved bytes/s = the algorithm's bytes (20 B per
parameter, + 2 B per shadowed element, + 2 B per transposed element) over the median window.

    python tools/bench_sgd.py [--calls 200] [--reps 10] [--out profiles/sgd.md]

Prints one JSON line and writes the table; profiles/sgd.md holds a recorded run.
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


def timed(fn, calls, reps, warmup=2):
    """Median / min / max microseconds per call of `fn` over `reps` event-bracketed windows of `calls` calls."""
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


def flat_grads(params, dev, seed):
    """.grad of every parameter = a view into one flat fp32 buffer of seeded noise (grad_sync.FlatGrads.setup's layout)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    flat = 1e-3 * torch.randn(sum(p.numel() for p in params), device=dev, generator=g)
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat


def sgd(groups, lr, **kw):
    opt = torch.optim.SGD(groups, lr=lr, momentum=0.9, nesterov=True, weight_decay=0.01, **kw)
    for g in opt.param_groups:
        g["lr"] = lr
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sgd.py measures on the GPU: none found")
    import vm_asr_amd
    from vm_asr_amd.fused_adamw import HipAdamWStep
    from vm_asr_amd.fused_sgd import HipSgdStep
    from vm_asr_amd.grad_guard import GradGuard
    from vm_asr_amd.optim import set_weight_decay
    dev = torch.device("cuda", 0)
    cfg = bench.make_config("vm_asr_48k_MPD", 4)
    torch.manual_seed(cfg.SEED)
    models = vm_asr_amd.get_model(cfg)
    res = {"workload": "vm_asr_48k_MPD parameter set", "device": torch.cuda.get_device_properties(dev).name, "calls": args.calls,
           "reps": args.reps}
    rows = []
    for name, key in (("generator", "generator"), ("mpd", "mpd")):
        model = models[key].to(dev)
        groups = set_weight_decay([model])
        params = [p for g in groups for p in g["params"]]
        flat_grads(params, dev, 1)
        n = sum(p.numel() for p in params)
        lr = torch.tensor(1e-6, device=dev)
        shadows = {id(p): p.detach().to(torch.bfloat16) for p in params}
        shadows_t = {id(p): p.detach().t().contiguous().to(torch.bfloat16) for p in params if p.dim() == 2}
        n_t = sum(p.numel() for p in params if p.dim() == 2)
        guard = GradGuard([p.grad for p in params], dev, None)
        guard.measure()
        fresh = lambda: [dict(g) for g in groups]      # noqa: E731
        out = {"parameters": n, "tensors": len(params), "transposed_elements": n_t}

        def record(label, t, nbytes):
            gbps = round(1e-3 * nbytes / t["median_us"], 1)
            out[label] = dict(t, GBps=gbps, bytes=nbytes)
            rows.append((name, label, t, nbytes, gbps))

        for label, sh, sht, gd in (("hip", None, None, None), ("hip + guard", None, None, guard), ("hip + shadows", shadows, shadows_t, None),
                                   ("hip + shadows + guard", shadows, shadows_t, guard)):
            step = HipSgdStep(sgd(fresh(), lr), sh, sht, guard=gd)
            out.setdefault("chunks", step.nchunks)
            record(label, timed(step.step, args.calls, args.reps), 20 * n + (2 * n + 2 * n_t if sh else 0))
        record("torch fused", timed(sgd(fresh(), lr, fused=True).step, max(1, args.calls // 10), args.reps), 20 * n)
        adam = torch.optim.AdamW(fresh(), lr=lr, capturable=True, fused=True)
        for g in adam.param_groups:
            g["lr"] = lr
        adam.step()
        record("hip adamw (28 B)", timed(HipAdamWStep(adam).step, args.calls, args.reps), 28 * n)
        assert guard.read()["skipped"] == 0 and all(bool(torch.isfinite(p).all()) for p in params)
        # last: torch's multi-tensor Nesterov step adds momentum * buf INTO the gradient tensors of a group without weight decay, so
        # repeated steps on one gradient compound it (the values overflow within a window; the time per call does not depend on them)
        record("torch foreach", timed(sgd(fresh(), lr, foreach=True).step, max(1, args.calls // 10), args.reps), 20 * n)
        res[name] = out
    print(json.dumps(res))
    lines = ["| model | parameters | step | median us | min | max | bytes | GB/s |", "|---|---|---|---|---|---|---|---|"]
    for name, label, t, nbytes, gbps in rows:
        lines.append(f"| {name} | {res[name]['parameters']} | {label} | {t['median_us']} | {t['min_us']} | {t['max_us']} | {nbytes} | {gbps} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(f"Recorded by tools/bench_sgd.py on {res['device']}: windows of {args.calls} calls (torch's own: {max(1, args.calls // 10)}), "
                 f"{args.reps} windows, device events.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
