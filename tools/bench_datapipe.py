"""What preparing a training batch on the device costs, measured on the GPU (Markdown sections for profiles/datapipe.md):

  --part design   `resample.design_on_device` against the host `resample.design` plus the fp32 cast and copy (`resample._taps`),
                  both directions of a rate coprime to 48 000 (960 001 taps each), caches emptied before every repetition; and,
                  for the ratios of tests/test_datapipe_gpu.py, how many device-designed taps differ from float32(host design).
  --part batch    `resample.degrade_batch` against the per-clip path of `resample.DegradeOnDevice` (degrade per clip, stack) for
                  batch 4 of one training segment at 48 kHz: 200 seeded random rates (50 batches) with caches emptied at the
                  start, and four fixed rates with warm caches.  Windows of batches between device synchronisations, host clock;
                  median [min, max] of the windows.  The outputs of the two paths are compared on the same inputs.

    timeout -k 10 300 python tools/bench_datapipe.py --part design --out design.md && \\
    timeout -k 10 600 python tools/bench_datapipe.py --part batch --out batch.md
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, SEGMENT_S, BATCH = 48000, 2.555, 4
COPRIME = (47999, 12347, 16001, 44101)                     # the rates of profiles/resample.md, "A ratio not seen before"
DESIGN = [(1, 3), (3, 1), (160, 147), (823, 3200), (3200, 823), (47999, 48000)]
FIXED = [16000, 24000, 12000, 8000]


def _sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _clear():
    from vm_asr_amd import resample
    resample._design.cache_clear()
    resample._device_taps.clear()
    resample._designed.clear()


def _fmt(v):
    return f"{statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]"


def part_design(reps=5):
    from vm_asr_amd import resample
    dev = torch.device("cuda", torch.cuda.current_device())
    resample.design_on_device(3, 1, dev), resample._taps(3, 1, dev)          # code objects loaded, allocator warm
    lines = ["## Filter design: device against host", "",
             f"Both directions of a rate coprime to 48 000 (two filters of 960 001 taps), caches emptied before each of {reps} "
             "repetitions, host clock around a device synchronise; median [min, max] in ms.  `host`: `resample.design` in float64 "
             "(numpy) + fp32 cast + host-to-device copy (`resample._taps`); `device`: `resample.design_on_device` (two launches per "
             "filter).", "", "| rate | host design + copy ms | design_on_device ms | ratio |", "|---|---|---|---|"]
    for r in COPRIME:
        host, devt = [], []
        for _ in range(reps):
            _clear()
            host.append(_sync_ms(lambda: (resample._taps(r, SR, dev), resample._taps(SR, r, dev))))
            _clear()
            devt.append(_sync_ms(lambda: (resample.design_on_device(r, SR, dev), resample.design_on_device(SR, r, dev))))
        lines.append(f"| {r} | {_fmt(host)} | {_fmt(devt)} | {statistics.median(host) / statistics.median(devt):.0f}x |")
    lines += ["", "Device-designed taps against the host design (the rule of tests/test_datapipe_gpu.py: |h_dev - h64| <= 2^-23 |h64| + "
              "1e-12 max|h64|):", "", "| up/down | taps | differ from float32(h64) | worst |h_dev - h64| / allowed |", "|---|---|---|---|"]
    for up, down in DESIGN:
        _clear()
        h64, _ = resample.design(up, down)
        h = resample.design_on_device(up, down, dev).cpu().numpy()
        allowed = 2.0 ** -23 * np.abs(h64) + 1e-12 * np.abs(h64).max()
        lines.append(f"| {up}/{down} | {h64.size} | {int((h != h64.astype(np.float32)).sum())} | "
                     f"{float((np.abs(h.astype(np.float64) - h64) / allowed).max()):.3f} |")
    return lines


def _per_clip(x, rates):
    """What DegradeOnDevice.__iter__ does with a batch on the device."""
    from vm_asr_amd import resample
    return torch.stack([resample.degrade(x[i], SR, r) for i, r in enumerate(rates)])


def _windows(fn, batches, per_window):
    """ms per batch of each window of `per_window` consecutive batches (a device synchronise on both sides)."""
    out = []
    for w in range(0, len(batches), per_window):
        chunk = batches[w:w + per_window]
        out.append(_sync_ms(lambda: [fn(r) for r in chunk]) / len(chunk))
    return out


def part_batch():
    from vm_asr_amd import resample
    T = int(SEGMENT_S * SR)
    x = 0.1 * torch.randn(BATCH, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    new, old = (lambda r: resample.degrade_batch(x, SR, r)), (lambda r: _per_clip(x, r))
    new([16000] * BATCH), old([16000] * BATCH)                                # code objects loaded, allocator warm
    rng = random.Random(0)
    cold = [[rng.randint(8000, 48000) for _ in range(BATCH)] for _ in range(50)]
    worst = 0.0
    for r in cold[:3]:                                                        # same inputs, both paths
        worst = max(worst, float((new(r) - old(r)).abs().max()))
    _clear()
    t_new = _windows(new, cold, 10)
    _clear()
    t_old = _windows(old, cold, 10)
    fixed = [FIXED] * 700
    new(FIXED), old(FIXED)
    w_new, w_old = _windows(new, fixed, 100), _windows(old, fixed, 100)
    w_new2, w_old2 = _windows(new, fixed, 100), _windows(old, fixed, 100)     # the same again: the spread between repetitions
    return ["## A batch of 4 at per-clip rates: degrade_batch against the per-clip path", "",
            f"x (4, {T}) fp32 on the device (one training segment, {SEGMENT_S} s at 48 kHz).  `per clip`: `torch.stack([degrade(x[i], 48000, "
            "r_i)])`, the body of `DegradeOnDevice.__iter__` (host design per new ratio, two launches + slice per clip, a stack); "
            "`degrade_batch`: filters designed on the device, two launches per batch.  ms per batch: median [min, max] over windows, "
            "host clock, a device synchronise on both sides of a window.", "",
            "| rates | windows | per clip ms | degrade_batch ms | ratio |", "|---|---|---|---|---|",
            f"| 200 random rates in [8000, 48000] (random.Random(0)), caches emptied first | 5 x 10 batches | {_fmt(t_old)} | {_fmt(t_new)} | "
            f"{statistics.median(t_old) / statistics.median(t_new):.0f}x |",
            f"| fixed {FIXED}, caches warm | 7 x 100 batches | {_fmt(w_old)} | {_fmt(w_new)} | "
            f"{statistics.median(w_old) / statistics.median(w_new):.1f}x |",
            f"| the same, repeated | 7 x 100 batches | {_fmt(w_old2)} | {_fmt(w_new2)} | "
            f"{statistics.median(w_old2) / statistics.median(w_new2):.1f}x |", "",
            f"Largest |degrade_batch - per clip| over the first three random batches: {worst:.3e} (signal rms 0.1)."]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["design", "batch"], required=True)
    ap.add_argument("--out", default=None, help="Markdown file to write (default: print only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_datapipe.py measures on the GPU"
    props = torch.cuda.get_device_properties(0)
    arch = getattr(props, "gcnArchName", "").split(":")[0]
    text = "\n".join((part_design if args.part == "design" else part_batch)()
                     + ["", f"(`python tools/bench_datapipe.py --part {args.part}` on {'MI355X' if arch == 'gfx950' else props.name} ({arch}), "
                        f"torch {torch.__version__}.)"]) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
