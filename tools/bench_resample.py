"""What the polyphase resampler costs, measured on the GPU (writes a Markdown report, profiles/resample.md):

  * time per `resample.resample_poly` call for 16 k -> 48 k, 48 k -> 16 k, 44.1 k -> 48 k, 48 k -> 12 345 and 12 345 -> 48 k at one
    training segment (DATA.SEGMENT of the 48 kHz configs: 2.555 s) and batch 4 — HIP events around windows of back-to-back calls
    (the call as a user issues it: launch included) and the library's own per-launch events (vmasr_prof_*: the kernel alone);
  * the algorithmic bytes (input + output + taps, each once) over the kernel time, against the HBM peak;
  * scipy.signal.resample_poly on the host for the same batch, when scipy is installed;
  * with --parity: max|hip - y64| over the allowed deviation for every case of tests/golden/resample.npz (the rule of
    tests/test_resample.py).

    python tools/bench_resample.py --out profiles/resample.md --parity
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X datasheet
SEGMENT_S, BATCH = 2.555, 4
RATES = [(16000, 48000), (48000, 16000), (44100, 48000), (48000, 12345), (12345, 48000)]


def _window_us(fn, calls, windows):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def measure(sr_from, sr_to, calls=200, windows=7):
    from vm_asr_amd import _lib, resample
    n_in = int(SEGMENT_S * sr_from)
    x = 0.1 * torch.randn(BATCH, n_in, device="cuda")
    fn = lambda: resample.resample_poly(x, sr_to, sr_from)   # noqa: E731
    for _ in range(20):
        y = fn()
    torch.cuda.synchronize()
    win = _window_us(fn, calls, windows)
    _lib.prof_enable(True)
    _lib.prof_reset()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    p = _lib.prof_collect()["resample_poly"]
    _lib.prof_enable(False)
    kern_us = p["ms"] * 1e3 / p["launches"]
    row = dict(sr_from=sr_from, sr_to=sr_to, n_in=n_in, n_out=y.shape[-1], taps=2 * resample.design(sr_to, sr_from)[1] + 1,
               call_us=statistics.median(win), call_lo=min(win), call_hi=max(win), kern_us=kern_us,
               bytes=p["alg_bytes"] / p["launches"], scipy_ms=None)
    try:
        from scipy.signal import resample_poly as sp
        xs = x.cpu().numpy()
        sp(xs, sr_to, sr_from, axis=-1)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            sp(xs, sr_to, sr_from, axis=-1)
            ts.append(time.perf_counter() - t0)
        row["scipy_ms"] = statistics.median(ts) * 1e3
    except ImportError:
        pass
    return row


def design_cost(rates=(47999, 12347, 16001, 44101), target=48000):
    """A ratio not seen before (DegradeOnDevice's random rates): host design + copy of both directions' filters, and the first
    degrade call including them, for rates coprime to the target (960 001 taps per direction)."""
    from vm_asr_amd import resample
    x = 0.1 * torch.randn(1, int(SEGMENT_S * target), device="cuda")
    rows = []
    for r in rates:
        resample._design.cache_clear()
        resample._device_taps.clear()
        t0 = time.perf_counter()
        h, _ = resample.design(r, target)
        resample.design(target, r)
        t1 = time.perf_counter()
        resample._taps(r, target, x.device), resample._taps(target, r, x.device)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        resample._design.cache_clear()
        resample._device_taps.clear()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        resample.degrade(x, target, r)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        resample.degrade(x, target, r)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        rows.append((r, h.size, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3))
    return rows


def parity_rows():
    from vm_asr_amd import resample
    g = np.load(os.path.join(ROOT, "tests", "golden", "resample.npz"))
    rows = []

    def add(what, got, y32, y64):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - y64).max())
        tol = max(4.0 * float(np.abs(y32.astype(np.float64) - y64).max()), 2.0 ** -23 * float(np.abs(y64).max()))
        rows.append((what, err, float(np.abs(y32.astype(np.float64) - y64).max()), tol, err / tol))
    for k in sorted(g.files):
        if k.startswith("x_"):
            fr, to, n = (int(v) for v in k[2:].split("_"))
            add(f"{fr} -> {to}, n_in {n}", resample.resample_poly(torch.from_numpy(g[k]).cuda(), to, fr), g["y32_" + k[2:]], g["y64_" + k[2:]])
        elif k.startswith("xp_"):
            fr, to, n = (int(v) for v in k[3:].split("_"))
            xp = g[k]
            y = resample.resample_poly(torch.from_numpy(np.tile(xp, (1, -(-n // xp.shape[1])))[:, :n]).cuda(), to, fr)
            if "y64_" + k[3:] in g.files:        # a strong decimation: whole output stored
                add(f"{fr} -> {to}, n_in {n}", y, g["y32_" + k[3:]], g["y64_" + k[3:]])
                continue
            add(f"{fr} -> {to}, n_in {n}, head", y[:, :256], g["y32h_" + k[3:]], g["y64h_" + k[3:]])
            add(f"{fr} -> {to}, n_in {n}, tail", y[:, -256:], g["y32t_" + k[3:]], g["y64t_" + k[3:]])
        elif k.startswith("deg_x_"):
            sr, si, n = (int(v) for v in k[6:].split("_"))
            add(f"degrade {sr} <-> {si}, n {n}", resample.degrade(torch.from_numpy(g[k]).cuda(), sr, si), g["deg_y32_" + k[6:]], g["deg_y64_" + k[6:]])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="Markdown report to write (default: print)")
    ap.add_argument("--parity", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py measures on the GPU"
    from vm_asr_amd.resample import CACHE_RATIOS
    torch.manual_seed(0)
    props = torch.cuda.get_device_properties(0)
    arch = getattr(props, "gcnArchName", "").split(":")[0]
    name = f"{'MI355X' if arch == 'gfx950' else props.name} ({arch}; torch names the device '{props.name}')"
    lines = ["# Polyphase resampler (csrc/resample.hip): measured cost and parity", "",
             f"`python tools/bench_resample.py --parity` on {name}, torch {torch.__version__}.", "",
             f"One training segment ({SEGMENT_S} s), batch {BATCH}, fp32.  `call`: HIP events around windows of 200 back-to-back "
             "`resample_poly` calls (median of 7 windows, [min, max]; launch and the output allocation included).  `kernel`: the "
             "library's per-launch events (vmasr_prof_*), mean of 200 launches.  `bytes`: input + output + taps, each once; "
             f"`of peak`: bytes / kernel time over {HBM_PEAK / 1e12:.1f} TB/s (HBM, datasheet).  `scipy`: "
             "scipy.signal.resample_poly on the host for the same batch (median of 5).", "",
             "| from -> to | n_in -> n_out | taps | call us | kernel us | bytes | GB/s | of peak | scipy ms |", "|---|---|---|---|---|---|---|---|---|"]
    for fr, to in RATES:
        r = measure(fr, to)
        bw = r["bytes"] / (r["kern_us"] * 1e-6)
        sc = "not measured (scipy absent)" if r["scipy_ms"] is None else f"{r['scipy_ms']:.2f}"
        lines.append(f"| {fr} -> {to} | {r['n_in']} -> {r['n_out']} | {r['taps']} | {r['call_us']:.1f} [{r['call_lo']:.1f}, {r['call_hi']:.1f}] | "
                     f"{r['kern_us']:.1f} | {r['bytes'] / 1e6:.2f} MB | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.1f} % | {sc} |")
    lines += ["", "## A ratio not seen before (the random rates of DegradeOnDevice's training branch)", "",
              f"One clip of {SEGMENT_S} s at 48 kHz degraded to a rate coprime to 48 000: two filters of 960 001 taps (down, up).  `design`: "
              "both filters in float64 on the host (sinc, np.kaiser); `copy`: fp32 cast and host-to-device copy of both; `first degrade`: "
              "the whole call with empty caches (design + copy + two kernels); `next degrade`: the same rate again (filters cached).  "
              f"The caches keep the {CACHE_RATIOS} most recently used ratios, so a run of "
              "random rates pays the first-call cost for most clips and holds a bounded amount of memory.", "",
              "| rate | taps per direction | design ms | copy ms | first degrade ms | next degrade ms |", "|---|---|---|---|---|---|"]
    lines += [f"| {r} | {n} | {d:.1f} | {c:.1f} | {f:.1f} | {s:.2f} |" for r, n, d, c, f, s in design_cost()]
    if args.parity:
        lines += ["", "## Parity against scipy (tests/golden/resample.npz, the rule of tests/test_resample.py)", "",
                  "allowed = max(4 max|y32 - y64|, 2^-23 max|y64|); y32 / y64 = scipy in fp32 / float64.", "",
                  "| case | max\\|hip - y64\\| | scipy fp32: max\\|y32 - y64\\| | allowed | used |", "|---|---|---|---|---|"]
        lines += [f"| {w} | {e:.2e} | {s:.2e} | {t:.2e} | {u:.2f} |" for w, e, s, t, u in parity_rows()]
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
