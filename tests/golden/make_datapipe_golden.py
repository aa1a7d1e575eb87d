"""Writes tests/golden/datapipe.npz: scipy.signal.resample_poly down, up and align on fixed batches at per-clip rates, for
tests/test_datapipe_gpu.py (the GPU tests read the file only: scipy need not be installed where they run).

    python tests/golden/make_datapipe_golden.py

Per case of CASES, `{name}`: `x_*` the fp32 batch (B, T), `rates_*` the input rate of each row (target rate SR), `y64_*` the
chain on the row widened to float64, `y32_*` the chain on the fp32 row (scipy then filters in fp32: its own fp32 error is the
yardstick of the tolerance, as in make_resample_golden.py).  The chain is the reference's degradation: resample_poly to the
row's rate, resample_poly back, trimmed or zero-padded to T; a row whose rate is SR is itself.  `full64_trim`: the untrimmed
float64 result of the 12 345 Hz row of the first case (2003 samples for T = 2000).  The long case keeps the file small: its
input is `xp_long` (one period per row) tiled to T, and only the first and last 256 outputs are stored (`y64h_*`, `y64t_*`,
`y32h_*`, `y32t_*`).
"""
import os

import numpy as np
from scipy.signal import resample_poly

HERE = os.path.dirname(os.path.abspath(__file__))

SR = 48000
CASES = [("b3_t2000", 2000, [16000, 12345, 48000]), ("b1_t2000", 2000, [12345]), ("b3_t7", 7, [16000, 12345, 48000])]
LONG = ("long", 50000, [47999, 16000])     # a 960 001-tap filter beside a 61-tap one
LONG_PERIOD, EDGE = 997, 256


def chain(x, rate, full=False):
    if rate == SR:
        return x.copy()
    y = resample_poly(resample_poly(x, rate, SR), SR, rate)
    n = x.shape[-1]
    if full:
        return y
    return y[:n] if y.shape[-1] >= n else np.pad(y, (0, n - y.shape[-1]))


def main():
    rng = np.random.default_rng(20250917)
    out = {}
    for name, T, rates in CASES:
        x = (0.1 * rng.standard_normal((len(rates), T))).astype(np.float32)
        out["x_" + name], out["rates_" + name] = x, np.array(rates, dtype=np.int64)
        out["y64_" + name] = np.stack([chain(x[b].astype(np.float64), r) for b, r in enumerate(rates)])
        out["y32_" + name] = np.stack([chain(x[b], r) for b, r in enumerate(rates)])
        assert out["y32_" + name].dtype == np.float32
    out["full64_trim"] = chain(out["x_b3_t2000"][1].astype(np.float64), 12345, full=True)
    assert out["full64_trim"].size == 2003
    name, T, rates = LONG
    xp = (0.1 * rng.standard_normal((len(rates), LONG_PERIOD))).astype(np.float32)
    x = np.tile(xp, (1, -(-T // LONG_PERIOD)))[:, :T]
    y64 = np.stack([chain(x[b].astype(np.float64), r) for b, r in enumerate(rates)])
    y32 = np.stack([chain(x[b], r) for b, r in enumerate(rates)])
    out["xp_" + name], out["rates_" + name] = xp, np.array(rates, dtype=np.int64)
    out["y64h_" + name], out["y64t_" + name] = y64[:, :EDGE], y64[:, -EDGE:]
    out["y32h_" + name], out["y32t_" + name] = y32[:, :EDGE], y32[:, -EDGE:]
    path = os.path.join(HERE, "datapipe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
