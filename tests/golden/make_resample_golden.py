"""Writes tests/golden/resample.npz: scipy.signal.resample_poly on fixed inputs, for tests/test_resample.py (the GPU tests read
the file only: scipy need not be installed where they run).

    python tests/golden/make_resample_golden.py

Per case `{sr_from}_{sr_to}_{n_in}` (batch 2, the rows differ):  `x_*` the fp32 input, `y64_*` scipy's result on the input
widened to float64, `y32_*` scipy's result on the fp32 input (scipy then filters in fp32: its own fp32 error is the yardstick
of the test's tolerance).  The long case keeps the file small: its input is `xp_*` (one period per row) tiled to n_in, and only
the first and last 256 outputs are stored (`y64h_*`, `y64t_*`, `y32h_*`, `y32t_*`).  `deg_*`: the degradation chain (down to
sr_input, up again, pad or trim to the input length) the same way.  The strong decimations (`STEEP`: the ratios at which the
kernel shrinks its tile or reads the input from global memory) need long inputs for a few hundred outputs: their inputs are
tiled periods too (`xp_*`), their outputs are stored whole (`y64_*`, `y32_*`).  `h_{up}_{down}`: the float64 taps scipy filters with,
up * firwin(...); for 3200/823 every 7th of the first half_len + 1 of the 64 001 symmetric taps (7 divides neither 3200 nor
823: the samples visit every polyphase branch).
"""
import math
import os

import numpy as np
from scipy.signal import firwin, resample_poly

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [(48000, 16000, 1000), (16000, 48000, 1000), (8000, 48000, 333), (48000, 8000, 1001), (48000, 44100, 700),
         (44100, 48000, 700), (12345, 48000, 500), (48000, 12345, 2000), (16000, 48000, 7), (48000, 16000, 7), (48000, 24000, 65)]
LONG = (48000, 47999, 50000)
LONG_PERIOD, EDGE = 997, 256
# 1/30: tile 128; 1/74: tile 64; 1/100: input window too large for any tile (x from global memory, 2001 taps staged);
# 1/500: x from global memory and the 10 001 taps read through L2
STEEP = [(48000, 1600, 10000), (7400, 100, 20000), (48000, 480, 30000), (48000, 96, 60000)]
DEGRADE = [(48000, 16000, 2000), (48000, 12345, 2000)]
TAPS = [(3, 1), (1, 6), (147, 160), (3200, 823)]


def taps(up, down):
    half_len = 10 * max(up, down)
    return up * firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)), half_len


def chain(x, sr, sr_input):
    y = resample_poly(resample_poly(x, sr_input, sr, axis=-1), sr, sr_input, axis=-1)
    n = x.shape[-1]
    return y[..., :n] if y.shape[-1] >= n else np.pad(y, ((0, 0), (0, n - y.shape[-1])))


def main():
    rng = np.random.default_rng(20240611)
    out = {}
    for fr, to, n in CASES:
        x = (0.1 * rng.standard_normal((2, n))).astype(np.float32)
        key = f"{fr}_{to}_{n}"
        out["x_" + key] = x
        out["y64_" + key] = resample_poly(x.astype(np.float64), to, fr, axis=-1)
        out["y32_" + key] = resample_poly(x, to, fr, axis=-1)
        assert out["y32_" + key].dtype == np.float32 and out["y64_" + key].shape[-1] == -(-n * to // fr)
    fr, to, n = LONG
    xp = (0.1 * rng.standard_normal((2, LONG_PERIOD))).astype(np.float32)
    x = np.tile(xp, (1, -(-n // LONG_PERIOD)))[:, :n]
    key = f"{fr}_{to}_{n}"
    y64, y32 = resample_poly(x.astype(np.float64), to, fr, axis=-1), resample_poly(x, to, fr, axis=-1)
    out["xp_" + key] = xp
    out["y64h_" + key], out["y64t_" + key] = y64[:, :EDGE], y64[:, -EDGE:]
    out["y32h_" + key], out["y32t_" + key] = y32[:, :EDGE], y32[:, -EDGE:]
    for sr, si, n in DEGRADE:
        x = (0.1 * rng.standard_normal((2, n))).astype(np.float32)
        key = f"{sr}_{si}_{n}"
        out["deg_x_" + key] = x
        out["deg_y64_" + key] = chain(x.astype(np.float64), sr, si)
        out["deg_y32_" + key] = chain(x, sr, si)
        assert out["deg_y32_" + key].dtype == np.float32
    for fr, to, n in STEEP:       # (after every other draw: the arrays above do not change when a case is added here)
        xp = (0.1 * rng.standard_normal((2, LONG_PERIOD))).astype(np.float32)
        x = np.tile(xp, (1, -(-n // LONG_PERIOD)))[:, :n]
        key = f"{fr}_{to}_{n}"
        out["xp_" + key] = xp
        out["y64_" + key] = resample_poly(x.astype(np.float64), to, fr, axis=-1)
        out["y32_" + key] = resample_poly(x, to, fr, axis=-1)
    for up, down in TAPS:
        assert math.gcd(up, down) == 1
        h, half_len = taps(up, down)
        assert np.array_equal(h, h[::-1])
        out[f"h_{up}_{down}"] = h if h.size < 8192 else h[:half_len + 1:7]
    path = os.path.join(HERE, "resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
