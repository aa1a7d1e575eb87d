"""The dense-tail convolution's test cases (tests/test_msd_tail_gpu.py runs them, tests/test_msd_tail.py checks what they reach) and
their float64 CPU references, computed once and shared (never modified)."""
import torch
import torch.nn.functional as F

# csrc/dconv1d.hip's tiles, mirrored so that the case list exists at collection time without the library:
# tests/test_msd_tail.py::test_case_list_reaches_the_tile_edges asserts that they are the library's.
POS_TILE, M_TILE, K_CHUNK = 128, 64, 16
P, M = POS_TILE, max(M_TILE, K_CHUNK)
GATE = 2e-5      # max|got - ref| <= 2e-5 max|ref| per tensor: the gate of the exact-fp32 MFMA convolutions (tests/test_msd_gpu.py)

# (B, Cin, Cout, L, k, pad)
WORKLOAD = (2, 1024, 1024, 30, 5, 2)       # the workload's channels at its shortest map
CONV_POST = (1, 1024, 1, 30, 3, 1)         # conv_post: act off only
CASES = [
    WORKLOAD,
    (3, 5, 3, 1, 5, 2),                    # L = 1
    (2, 7, 18, 2, 5, 2),
    (1, 20, 17, P + 1, 5, 2),              # one position past the largest position tile
    (2, M + 1, M + 1, 9, 3, 1),            # one channel past the M tile (both GEMMs) and past a K chunk: a last chunk of ONE channel
    (2, 6, 4, 5, 5, 0),                    # pad 0, T = 1
    (1, 3, 2, 4, 5, 4),                    # pad k - 1, T > L
    (2, 8, 8, 16, 1, 0),                   # pointwise
    # beyond the issue's list: the other two position tiles' edges (<= 32: 2 tiles of 16, <= 64: 4, else 8), 33 channels (a second,
    # one-channel tile of the weight gradient's 32), the most taps, and B 2 x T 69: K units (b, 32 outputs) whose last one is short
    (1, 20, 17, 33, 5, 2),
    (2, 33, 17, 70, 8, 3),
]
NO_BIAS = (2, 7, 18, 2, 5, 2, "nobias")    # the one case without a bias

_REF = {}


def problem(case, act):
    """-> (x, w, b or None, gy, y64, dx64, dw64, db64 or None) of one case: seeded inputs of unit scale, float64 autograd on the CPU."""
    key = (case, act)
    if key not in _REF:
        B, Cin, Cout, L, k, pad = case[:6]
        bias = len(case) == 6
        g = torch.Generator().manual_seed(7000 + 131 * Cin + 17 * Cout + L + 3 * k + pad + (0 if bias else 1))
        x = torch.randn(B, Cin, L, generator=g)
        w = torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
        b = torch.randn(Cout, generator=g) if bias else None
        gy = torch.randn(B, Cout, L + 2 * pad - k + 1, generator=g)
        x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
        b64 = b.double().requires_grad_() if bias else None
        y64 = F.conv1d(x64, w64, b64, 1, pad)
        if act:
            y64 = F.gelu(y64)
        y64.backward(gy.double())
        _REF[key] = (x, w, b, gy, y64.detach(), x64.grad, w64.grad, b64.grad if bias else None)
    return _REF[key]
