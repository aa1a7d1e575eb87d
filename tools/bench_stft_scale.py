"""Microbenchmark: the STFT / iSTFT front-end (csrc/stft.hip) under the two spectrogram scales (dev tool).

    python tools/bench_stft_scale.py [--scale log2|dB|both] [--batch 4] [--length 122640] [--n-fft 1024] [--hop 240] [--win 1024]

Times wav2spectro, spectro2wav and spectro2wav's backward.  Each figure is the time of one call inside a replayed HIP graph of
--calls calls (an eager call of this size measures the launch path), taken --reps times with device events; the scales alternate
replay by replay so that drift hits both.  Prints median, 10th and 90th percentile in microseconds, and one JSON line."""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vm_asr_amd import stft

dev = torch.device("cuda:0")


def capture(fn, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_alternating(graphs, calls, reps):
    """{name: [us per call] * reps}, the graphs replayed in turn."""
    out = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / calls * 1e3)
    return out


def stats(v):
    t = torch.tensor(v, dtype=torch.float64)
    return dict(median=t.median().item(), p10=t.quantile(0.1).item(), p90=t.quantile(0.9).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", choices=["log2", "dB", "both"], default="both")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--length", type=int, default=122640)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=240)
    ap.add_argument("--win", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    scales = ["log2", "dB"] if a.scale == "both" else [a.scale]
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(a.batch, 1, a.length, generator=g)).to(dev)
    result = dict(batch=a.batch, length=a.length, n_fft=a.n_fft, hop=a.hop, win=a.win, calls=a.calls, reps=a.reps, us={})
    F, M = a.n_fft // 2 + 1, 1 + a.length // a.hop
    print(f"B {a.batch} T {a.length} n_fft {a.n_fft} hop {a.hop} win {a.win}: maps of {a.batch * F * M * 4 / 1e6:.1f} MB each")
    fwd, inv, bwd = {}, {}, {}
    keep = []
    for s in scales:
        mag, ph = stft.wav2spectro(wave, a.n_fft, a.hop, a.win, s)
        m, p = mag.clone().requires_grad_(), ph.clone().requires_grad_()
        gw = torch.randn_like(stft.spectro2wav(mag, ph, a.n_fft, a.hop, a.win, s))
        keep.append((m, p, gw))
        fwd[s] = capture(lambda s=s: stft.wav2spectro(wave, a.n_fft, a.hop, a.win, s), a.calls)
        with torch.no_grad():
            inv[s] = capture(lambda s=s, mag=mag, ph=ph: stft.spectro2wav(mag, ph, a.n_fft, a.hop, a.win, s), a.calls)

        def both(s=s, m=m, p=p, gw=gw):
            m.grad = p.grad = None
            stft.spectro2wav(m, p, a.n_fft, a.hop, a.win, s).backward(gw)
        bwd[s] = capture(both, a.calls)
    for name, graphs in (("wav2spectro", fwd), ("spectro2wav", inv), ("spectro2wav fwd+bwd", bwd)):
        t = time_alternating(graphs, a.calls, a.reps)
        for s in scales:
            st = stats(t[s])
            result["us"][f"{name} {s}"] = st
            print(f"{name:22s} {s:5s}: median {st['median']:7.1f} us   p10 {st['p10']:7.1f}   p90 {st['p90']:7.1f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
