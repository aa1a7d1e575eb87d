"""Microbenchmark: MultiResolutionSTFTLoss(emphasize_high_freq=True), fused kernels against the composed ATen path (dev tool).

    python tools/bench_stftloss.py [--batch 4] [--length 122640] [--calls 200] [--reps 30] [--plain]
    python tools/bench_stftloss.py --count [--plain]          # launch counts instead of times (a run of its own: profiler on)

One call = forward + backward of the three-resolution loss on a (batch, length) pair.  The two arms are the same module with
VMASR_STFT_LOSS=1 (csrc/stftloss.hip: the weighted forward / finish / backward) and VMASR_STFT_LOSS=0 (stft_magnitude twice, sub,
norms, logs, l1_loss: what the flag ran before the weighted kernels existed); the switch is read per call, so both run in ONE
process and alternate window by window — drift and neighbours on the machine hit both.  A window is --calls calls issued by
the host between two device events, after a warm-up of every arm: the time of an eager call, launch path included, which is
what the ~170 small launches of the composed path cost an eager train step.  Both STFT passes are inside either arm, so the
difference is the loss arithmetic alone.  Prints median, 10th and 90th percentile per arm in microseconds per call, the spread
of the fused arm against itself (the medians of its even and of its odd windows) and one JSON line.  --count does not time:
it prints the device-side launches of one call of every arm as torch.profiler reports them.  --plain adds
emphasize_high_freq=False (its fused arm differs by the weight alone).  Replay from a HIP graph is not measured here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vm_asr_amd.loss import MultiResolutionSTFTLoss

dev = torch.device("cuda:0")
ARMS = (("fused", "1"), ("composed", "0"))


def make_step(L, x, y, knob):
    def step():
        os.environ["VMASR_STFT_LOSS"] = knob
        x.grad = None
        sc, mag = L(x, y)
        (sc + mag).backward()
        return sc.detach(), mag.detach()
    return step


def time_alternating(runs, calls, reps):
    """{name: [us per call] * reps}; runs[name]() issues `calls` calls; the arms take turns."""
    out = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / calls * 1e3)
    return out


def stats(v):
    t = torch.tensor(v, dtype=torch.float64)
    return dict(median=t.median().item(), p10=t.quantile(0.1).item(), p90=t.quantile(0.9).item())


def count_launches(step):
    """Kernels (and copies / memsets) on the device during one call, from torch.profiler."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    if not names:
        raise RuntimeError("torch.profiler reported no device-side event")
    other = sum(1 for n in names if n.lower().startswith(("memcpy", "memset")))
    return dict(kernels=len(names) - other, copies_memsets=other, stft_loss_kernels=sum(1 for n in names if "stft_loss" in n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--length", type=int, default=122640)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--plain", action="store_true", help="also emphasize_high_freq=False")
    ap.add_argument("--count", action="store_true", help="count the launches of one call with torch.profiler instead of timing")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    y = (0.1 * torch.randn(a.batch, a.length, generator=g)).to(dev)
    x = (y + 0.03 * torch.randn(a.batch, a.length, generator=g).to(dev)).requires_grad_()
    mods = {"emph": MultiResolutionSTFTLoss(emphasize_high_freq=True).to(dev)}
    if a.plain:
        mods["plain"] = MultiResolutionSTFTLoss(emphasize_high_freq=False).to(dev)
    steps = {f"{m} {arm}": make_step(L, x, y, knob) for m, L in mods.items() for arm, knob in ARMS}
    result = dict(batch=a.batch, length=a.length, calls=a.calls, reps=a.reps, us={}, launches={}, values={})
    print(f"B {a.batch} T {a.length}: forward + backward of 3 resolutions, {a.calls} calls per timed window, {a.reps} windows per arm")
    for k, step in steps.items():                      # warm-up of every arm; the two arms must agree before they are compared
        for _ in range(3):
            sc, mag = step()
        torch.cuda.synchronize()
        result["values"][k] = dict(sc=sc.item(), mag=mag.item(), grad_absmax=x.grad.abs().max().item())
        print(f"{k:16s}: sc {sc.item():.7f} mag {mag.item():.7f} max|dx| {x.grad.abs().max().item():.4e}")
    if a.count:
        for k, step in steps.items():
            result["launches"][k] = count_launches(step)
            print(f"launches per call, {k:16s}: {result['launches'][k]}")
        print(json.dumps(result))
        return

    def eager(step):
        def run():
            for _ in range(a.calls):
                step()
        return run

    t = time_alternating({k: eager(s) for k, s in steps.items()}, a.calls, a.reps)
    for k in steps:
        st = stats(t[k])
        result["us"][k] = st
        print(f"{k:16s}: median {st['median']:8.1f} us   p10 {st['p10']:8.1f}   p90 {st['p90']:8.1f}")
    f = t["emph fused"]
    ha, hb = stats(f[0::2])["median"], stats(f[1::2])["median"]
    result["us"]["emph fused even / odd windows"] = [ha, hb]
    print(f"emph fused against itself (even / odd windows): {ha:.1f} / {hb:.1f} us, spread {abs(ha - hb) / min(ha, hb) * 100:.1f} %")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
