"""Times the multi-scale discriminator's grouped convolutions, `hip` (csrc/gconv1d.hip) against `torch` (F.conv1d), its stem (`--stem`:
csrc/stem1d.hip against F.gelu(F.conv1d), gelu_backward and aten.convolution_backward), its dense tail (`--tail`: csrc/dconv1d.hip
against the same operators) and the eager ["mpd", "msd"] train step.  One process, one device.  Every figure compares the two routes in the same call, ALTERNATING them: after
warm-up calls of both, `--rounds` rounds of (hip window, torch window); a window is n back-to-back calls between two HIP events, n
chosen per route so that a window lasts about `--window-ms`; the figure of a window is its time / n.  Reported per route: the median,
the minimum and the maximum of the windows (the spread: a difference inside it is not one).  profiles/msd.md and profiles/msd_stem.md
hold the output.

    python tools/bench_msd.py [--batch 4] [--samples 122640] [--rounds 7] [--window-ms 100] [--step] [--out FILE]
    python tools/bench_msd.py --stem [--step] [...]     # the stem at the three scale lengths, B 4 and 8; --step alternates VMASR_MSD_STEM
    python tools/bench_msd.py --tail [--step] [...]     # convs.6 and conv_post at the three map lengths, B 8 and 4 (profiles/msd_tail.md);
                                                        # --step alternates VMASR_MSD_TAIL
    python tools/bench_msd.py --featmatch [--step] [...]  # the generator's MSD pass with its feature-matching loss (profiles/msd_featmatch.md);
                                                          # --step alternates VMASR_MSD_FEAT
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, S, PAD = 41, 4, 20


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def compare(fns, rounds, window_ms, warmup=3, max_calls=4000):
    """fns: {route: callable}.  -> {route: {"ms": median, "min": ..., "max": ..., "calls": n per window}} from alternated windows."""
    n = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        n[k] = max(1, min(max_calls, int(window_ms / max(_window(fn, 3), 1e-4))))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_window(fn, n[k]))
    return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v), "calls": n[k]} for k, v in ms.items()}


def layer_rows(batch, samples, rounds, window_ms, hidden=128):
    from vm_asr_amd import msd_ops
    h = hidden
    layers = [(h, h, 4), (h, 2 * h, 16), (2 * h, 4 * h, 16), (4 * h, 8 * h, 16), (8 * h, 8 * h, 16)]
    L, rows = samples, []
    g_in = torch.ops.aten.gelu_backward
    for li, (ci, co, g) in enumerate(layers, start=1):
        T = (L + 2 * PAD - K) // S + 1
        x = torch.randn(batch, ci, L, device="cuda")
        w = torch.randn(co, ci // g, K, device="cuda") / (ci // g * K) ** 0.5
        b = torch.randn(co, device="cuda")
        gy = torch.randn(batch, co, T, device="cuda")
        y, pre = msd_ops.gconv1d_fwd(x, w, b, g, S, PAD, True)
        gflop = 2.0 * batch * co * T * (ci // g) * K / 1e9
        row = {"layer": f"convs.{li}", "Cin": ci, "Cout": co, "groups": g, "L": L, "T": T, "gflop": round(gflop, 2)}
        ops = {
            "fwd": {"hip": lambda: msd_ops.gconv1d_fwd(x, w, b, g, S, PAD, True), "torch": lambda: F.gelu(F.conv1d(x, w, b, S, PAD, 1, g))},
            "dgrad": {"hip": lambda: msd_ops.gconv1d_dgrad(gy, pre, w, x.shape, g, S, PAD),
                      "torch": lambda: torch.ops.aten.convolution_backward(g_in(gy, pre), x, w, [co], [S], [PAD], [1], False, [0], g,
                                                                           [True, False, False])},
            "wgrad": {"hip": lambda: msd_ops.gconv1d_wgrad(x, gy, pre, w.shape, g, S, PAD),
                      "torch": lambda: torch.ops.aten.convolution_backward(g_in(gy, pre), x, w, [co], [S], [PAD], [1], False, [0], g,
                                                                           [False, True, True])},
        }
        for op, fns in ops.items():
            for route, r in compare(fns, rounds, window_ms).items():
                row[f"{route}_{op}_ms"], row[f"{route}_{op}_min"], row[f"{route}_{op}_max"] = r["ms"], r["min"], r["max"]
                row[f"{route}_{op}_calls"] = r["calls"]
        rows.append(row)
        L = T
    return rows


STEM_K, STEM_PAD, STEM_LENGTHS, STEM_BATCHES = 15, 7, (122640, 61321, 30661), (4, 8)


def stem_rows(rounds, window_ms, hidden=128):
    """The stem (1 -> hidden, k 15, stride 1, pad 7) at the three scale lengths: forward, backward for dw + db (the discriminator's
    pass), backward for dx alone (the generator's pass).  GB/s: the fused route's own minimal traffic (the map once + x + the taps)."""
    from vm_asr_amd import msd_ops
    g_in, rows = torch.ops.aten.gelu_backward, []
    for batch in STEM_BATCHES:
        for L in STEM_LENGTHS:
            x = torch.randn(batch, 1, L, device="cuda")
            w = torch.randn(hidden, 1, STEM_K, device="cuda") / STEM_K ** 0.5
            b = torch.randn(hidden, device="cuda")
            gy = torch.randn(batch, hidden, L, device="cuda")
            pre = F.conv1d(x, w, b, 1, STEM_PAD)

            def cb(mask):
                return torch.ops.aten.convolution_backward(g_in(gy, pre), x, w, [hidden], [1], [STEM_PAD], [1], False, [0], 1, mask)
            small = 4.0 * (batch * L + hidden * (STEM_K + 1))
            nbytes = {"fwd": 4.0 * gy.numel() + small, "bwd_w": 4.0 * gy.numel() + small, "bwd_x": 4.0 * gy.numel() + small + 4.0 * batch * L}
            ops = {
                "fwd": {"hip": lambda: msd_ops.stem1d_fwd(x, w, b, STEM_PAD, True), "torch": lambda: F.gelu(F.conv1d(x, w, b, 1, STEM_PAD))},
                "bwd_w": {"hip": lambda: msd_ops.stem1d_bwd(gy, x, w, b, STEM_PAD, True, False, True, True),
                          "torch": lambda: cb([False, True, True])},
                "bwd_x": {"hip": lambda: msd_ops.stem1d_bwd(gy, x, w, b, STEM_PAD, True, True, False, False),
                          "torch": lambda: cb([True, False, False])},
            }
            row = {"layer": "convs.0", "B": batch, "Cout": hidden, "L": L, "map_MB": round(4.0 * gy.numel() / 1e6, 1)}
            for op, fns in ops.items():
                for route, r in compare(fns, rounds, window_ms).items():
                    row[f"{route}_{op}_ms"], row[f"{route}_{op}_min"], row[f"{route}_{op}_max"] = r["ms"], r["min"], r["max"]
                    row[f"{route}_{op}_calls"] = r["calls"]
                row[f"hip_{op}_GBps"] = round(nbytes[op] / row[f"hip_{op}_ms"] / 1e6, 1)
            rows.append(row)
            del x, w, b, gy, pre
    return rows


TAIL_LENGTHS, TAIL_LAYERS = (120, 60, 30), (("convs.6", 8, 5, 2, True), ("conv_post", 0, 3, 1, False))
F32_MATRIX_PEAK_TFLOPS = 157.3      # MI355X, dense fp32 matrix (v_mfma_f32_16x16x4_f32: 256 FLOP / cycle / CU, 256 CUs, 2.4 GHz)


def tail_rows(rounds, window_ms, hidden=128):
    """The dense tail (8h -> 8h k 5 + GELU; conv_post 8h -> 1 k 3) at the workload's map lengths: B 8 (the discriminator's stacked
    pass: forward, dgrad, wgrad) and B 4 (the generator's pass: forward, dgrad).  pct_peak: the hip route's share of the fp32 matrix peak."""
    from vm_asr_amd import msd_ops
    g_in, rows, C = torch.ops.aten.gelu_backward, [], 8 * hidden
    for name, co_mul, k, pad, act in TAIL_LAYERS:
        co = co_mul * hidden or 1
        for batch, op_names in ((8, ("fwd", "dgrad", "wgrad")), (4, ("fwd", "dgrad"))):
            for L in TAIL_LENGTHS:
                x = torch.randn(batch, C, L, device="cuda")
                w = torch.randn(co, C, k, device="cuda") / (C * k) ** 0.5
                b = torch.randn(co, device="cuda")
                gy = torch.randn(batch, co, L, device="cuda")
                pre = msd_ops.dconv1d_fwd(x, w, b, 1, pad, act)[1]

                def cb(mask):
                    return torch.ops.aten.convolution_backward(g_in(gy, pre) if act else gy, x, w, [co], [1], [pad], [1], False, [0], 1, mask)
                ops = {
                    "fwd": {"hip": lambda: msd_ops.dconv1d_fwd(x, w, b, 1, pad, act),
                            "torch": (lambda: F.gelu(F.conv1d(x, w, b, 1, pad))) if act else (lambda: F.conv1d(x, w, b, 1, pad))},
                    "dgrad": {"hip": lambda: msd_ops.dconv1d_dgrad(gy, pre, w, x.shape, 1, pad), "torch": lambda: cb([True, False, False])},
                    "wgrad": {"hip": lambda: msd_ops.dconv1d_wgrad(x, gy, pre, w.shape, 1, pad), "torch": lambda: cb([False, True, True])},
                }
                gflop = 2.0 * batch * co * L * C * k / 1e9
                row = {"layer": name, "B": batch, "Cin": C, "Cout": co, "L": L, "k": k, "gflop": round(gflop, 3)}
                for op in op_names:
                    for route, r in compare(ops[op], rounds, window_ms).items():
                        row[f"{route}_{op}_ms"], row[f"{route}_{op}_min"], row[f"{route}_{op}_max"] = r["ms"], r["min"], r["max"]
                        row[f"{route}_{op}_calls"] = r["calls"]
                    row[f"hip_{op}_pct_peak"] = round(100.0 * gflop / row[f"hip_{op}_ms"] / F32_MATRIX_PEAK_TFLOPS, 2)
                rows.append(row)
                del x, w, b, gy, pre
    tot = {r: sum(v for row in rows for n, v in row.items() if n.startswith(r + "_") and n.endswith("_ms")) for r in ("hip", "torch")}
    spread = {r: sum(row[n[:-3] + "_max"] - row[n[:-3] + "_min"] for row in rows for n in row if n.startswith(r + "_") and n.endswith("_ms"))
              for r in ("hip", "torch")}
    rows.append({"layer": "sum of the medians", "hip_ms": tot["hip"], "torch_ms": tot["torch"], "hip_spread_ms": spread["hip"],
                 "torch_spread_ms": spread["torch"]})
    return rows


def featmatch_rows(batch, samples, rounds, window_ms, hidden=128):
    """The generator's pass through the MSD (forward_generator: scores + feature-matching loss, backward to the waveform; training mode,
    so a power iteration per weight as in the trainer) with VMASR_MSD_FEAT at hip and at torch on the same tensors; then one pass per
    route for its peak of allocated memory above the resident tensors, and the two routes' loss and dx against each other."""
    from vm_asr_amd.msd import MultiScaleDiscriminator
    torch.manual_seed(0)
    D = MultiScaleDiscriminator(hidden=hidden).cuda().train()
    real = 0.3 * torch.randn(batch, 1, samples, device="cuda")
    x = (0.3 * torch.randn(batch, 1, samples, device="cuda")).requires_grad_()
    with torch.no_grad():
        _, f_real = D.forward_single(real, detach_weights=True)

    def gen_pass(mode):
        os.environ["VMASR_MSD_FEAT"] = mode
        scores, loss = D.forward_generator(x, f_real)
        (2.0 * loss + sum((s ** 2).mean() for s in scores)).backward()
        g, x.grad = x.grad, None
        return loss.detach(), g

    row = {"pass": "generator", "B": batch, "hidden": hidden, "T": samples, "maps_MB": round(sum(4.0 * f.numel() for fs in f_real for f in fs) / 1e6, 1)}
    for route, r in compare({"hip": lambda: gen_pass("hip"), "torch": lambda: gen_pass("torch")}, rounds, window_ms).items():
        row[f"{route}_ms"], row[f"{route}_min"], row[f"{route}_max"], row[f"{route}_calls"] = r["ms"], r["min"], r["max"], r["calls"]
    uv = {k: v.clone() for k, v in D.state_dict().items() if k.endswith("._u") or k.endswith("._v")}
    out = {}
    for route in ("hip", "torch"):
        D.load_state_dict(uv, strict=False)        # the same weights for both routes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out[route] = gen_pass(route)
        torch.cuda.synchronize()
        row[f"{route}_peak_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
    (lh, gh), (lt, gt) = out["hip"], out["torch"]
    row["loss_hip"], row["loss_torch"] = lh.item(), lt.item()
    row["loss_rel_err"] = abs(lh.item() - lt.item()) / abs(lt.item())
    row["dx_err_of_max"] = ((gh - gt).abs().max() / gt.abs().max()).item()
    os.environ.pop("VMASR_MSD_FEAT")
    return [row]


def step_ms(batch, samples, rounds, steps=4, knob="VMASR_MSD_CONV"):
    """One trainer; `knob` (VMASR_MSD_CONV, or VMASR_MSD_STEM / VMASR_MSD_TAIL for the stem / the dense tail alone) is read at every call, so the two routes alternate
    in windows of `steps` steps on the same state."""
    from vm_asr_amd import get_model
    from vm_asr_amd.config import get_default_config, update_config
    from vm_asr_amd.trainer import SyntheticVCTK, Trainer, build_optimizer
    c = get_default_config()           # bench.py's vm_asr_48k_MPD workload with the MSD listed beside the MPD
    c.MODEL.NAME = "DualStreamInteractiveMambaUNet"
    c.TRAIN.LOW_FREQ_REPLACEMENT = True
    c.DATA.TARGET_SR = 48000
    c.DATA.LPF.MULTIFILTER = True
    c.TRAIN.ADVERSARIAL.ENABLE = True
    c.TRAIN.ADVERSARIAL.DISCRIMINATORS = ["mpd", "msd"]
    c.DATA.BATCH_SIZE = batch
    config = update_config(c)
    torch.manual_seed(config.SEED)
    models = get_model(config)
    dev = torch.device("cuda:0")
    opts = {"generator": build_optimizer(config, models["generator"]),
            "discriminator": build_optimizer(config, [models["mpd"], models["msd"]])}
    tr = Trainer(models, [], opts, config, dev, None, None, {}, amp=True, gan=True, len_epoch=0, dp_mode="flat")
    for m in tr.models.values():
        m.train()
    ds = SyntheticVCTK(config, length=batch, sr_in=16000, seed=123)
    inp, tgt, hc = next(iter(torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=False)))[:3]
    wave_in, wave, hf = inp.to(dev), tgt.to(dev), hc.to(dev)
    ms = {"hip": [], "torch": []}
    for mode in ms:                    # warm-up of both routes
        os.environ[knob] = mode
        for _ in range(3):
            tr.train_step(wave_in, wave, hf)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for mode in ms:
            os.environ[knob] = mode
            ms[mode].append(_window(lambda: tr.train_step(wave_in, wave, hf), steps))
    os.environ.pop(knob)
    return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v), "calls": steps} for k, v in ms.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--samples", type=int, default=122640)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--step", action="store_true", help="also time the eager ['mpd', 'msd'] train step, hip and torch alternated")
    ap.add_argument("--stem", action="store_true", help="time the stem (csrc/stem1d.hip) instead of the grouped layers; --step then alternates VMASR_MSD_STEM")
    ap.add_argument("--tail", action="store_true", help="time the dense tail (csrc/dconv1d.hip) instead of the grouped layers; --step then alternates VMASR_MSD_TAIL")
    ap.add_argument("--featmatch", action="store_true", help="time the generator's MSD pass with its feature-matching loss, VMASR_MSD_FEAT "
                    "hip and torch alternated, instead of the layers; --step then alternates VMASR_MSD_FEAT")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.featmatch:
        rows, knob = featmatch_rows(a.batch, a.samples, a.rounds, a.window_ms), "VMASR_MSD_FEAT"
    elif a.tail:
        rows, knob = tail_rows(a.rounds, a.window_ms), "VMASR_MSD_TAIL"
    elif a.stem:
        rows, knob = stem_rows(a.rounds, a.window_ms), "VMASR_MSD_STEM"
    else:
        rows, knob = layer_rows(a.batch, a.samples, a.rounds, a.window_ms), "VMASR_MSD_CONV"
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "samples": a.samples, "rounds": a.rounds, "window_ms": a.window_ms,
           "layers": rows}
    for r in res["layers"]:
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) and abs(v) >= 1e-3 else v) for k, v in r.items()}), flush=True)
    if a.step:
        res["step"] = step_ms(a.batch, a.samples, a.rounds, knob=knob)
        print(json.dumps({"step": {k: {n: round(x, 2) for n, x in v.items()} for k, v in res["step"].items()}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
