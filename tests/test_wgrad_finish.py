"""The end-of-pass finish of the weight gradients (csrc/wgrad.hip: vmasr_wgrad_finish_multi, queued by vm_asr_amd/wgrad.py) and of
LayerNorm's dgamma / dbeta (csrc/ln.hip: vmasr_layer_norm_bwd_reduce_multi) on their own terms: the C ABI contract, each kernel
against its definition, refusal before any launch, and the host queue's lifetime rules.

Every kernel output is held to two requirements, elementwise:

  bit-exact   wgrad finish: s = 0; for j in range(S): s += parts[j] in fp32 (the kernel's contract is a fixed summation order over
              the slabs and the library is built without fast-math, so equality is the requirement).  LayerNorm reduce: what
              vmasr_layer_norm_bwd's own one-item reduction writes for the same partials (both kernels add the same partials in
              the same lane order).
  float64     |got - sum64| <= n * 2^-24 * sum |terms|, n = S (slabs) or nblk (partials): the first-order bound of an fp32 sum of n
              terms in any order.  Derived, not measured.

A GEMM's weight gradient against gy^T x in float64 is held to  rows * 2^-24 * sum_r |gy[r] x[r]|: `rows` fp32 terms (products of
fp32 inputs rounded once, or fused) added in any order, which also covers the split into slabs and their sum.  Where autograd adds
two such gradients the bound is (rows + 1) * 2^-24 * (sum of both): one more rounding of a sum no larger than the terms' magnitudes.

Outputs live inside larger buffers filled with a canary; every float outside the outputs must still hold it.  Padding columns of
the partials (ld > cols) hold 1e30, so a read of the wrong column shows.  Achieved errors: profiles/wgrad_finish.md.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vmasr_hip.h")
DEV = "cuda"
U = 2.0 ** -24          # unit roundoff of fp32
CANARY = -12345.678     # (rounded to fp32 by torch.full: compared with the same rounded value)
GAP = 19                # canary floats before, between and after the outputs of an item (odd: outputs are not 16-byte aligned)


# ---- CPU: C ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_prototyped():
    from vm_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("vmasr_wgrad_finish_multi", 11), ("vmasr_layer_norm_bwd_reduce_multi", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == nargs, name


_P = 64   # any non-null address: a refused call dereferences nothing behind it


def _ptrs(*vals):
    return np.array(vals, dtype=np.uint64)


def _i32(*vals):
    return np.array(vals, dtype=np.int32)


#                                  parts dw  db  e1 e2 S  N  K  ld   (item 1 of 2; item 0 is always good)
_WG_GOOD = dict(parts=_P, dw=_P, db=_P, e1=0, e2=0, S=2, N=3, K=4, ld=5)


@pytest.mark.parametrize("change", [
    dict(n=0), dict(null="parts"), dict(null="dws"), dict(null="dbs"), dict(parts=0), dict(dw=0), dict(S=0), dict(N=0), dict(K=0),
    dict(db=0, ld=3), dict(ld=4), dict(e1=_P, ld=5), dict(e1=_P, e2=_P, ld=6),        # ld one less than K + (db) + (e1) + (e2)
    dict(db=0, e1=_P, ld=8), dict(e2=_P, ld=8),                                        # e1 without db, e2 without e1
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_wgrad_finish_contract_violations_return_einval_before_any_launch(change):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    a = dict(_WG_GOOD, **{k: v for k, v in change.items() if k not in ("n", "null")})
    cols = {k: np.array([_WG_GOOD[k], a[k]], dtype=np.uint64 if k in ("parts", "dw", "db", "e1", "e2") else np.int32)
            for k in _WG_GOOD}
    arrs = dict(parts=cols["parts"], dws=cols["dw"], dbs=cols["db"], e1s=cols["e1"], e2s=cols["e2"], Ss=cols["S"], Ns=cols["N"],
                Ks=cols["K"], lds=cols["ld"])
    args = [None if change.get("null") == k else v.ctypes.data for k, v in arrs.items()]
    code = lib.vmasr_wgrad_finish_multi(*args, change.get("n", 2), None)
    assert code == -1
    assert b"wgrad_finish_multi" in lib.vmasr_last_error(), lib.vmasr_last_error()


@pytest.mark.parametrize("change", [dict(n=0), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4), dict(part=0),
                                    dict(nblk=0), dict(C=0), dict(C=1025)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_layer_norm_reduce_contract_violations_return_einval_before_any_launch(change):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    parts, dgs, dbs = _ptrs(_P, change.get("part", _P)), _ptrs(_P, _P), _ptrs(_P, _P)
    nblk, Cs = _i32(3, change.get("nblk", 3)), _i32(8, change.get("C", 8))
    args = [a.ctypes.data for a in (parts, dgs, dbs, nblk, Cs)]
    if "null" in change:
        args[change["null"]] = None
    code = lib.vmasr_layer_norm_bwd_reduce_multi(*args, change.get("n", 2), None)
    assert code == -1
    assert b"layer_norm_bwd_reduce_multi" in lib.vmasr_last_error(), lib.vmasr_last_error()


# ---- helpers of the GPU tests ---------------------------------------------------------------------------------------------------------
ACHIEVED = {}     # case group -> largest |got - sum64| / bound seen (printed per test; profiles/wgrad_finish.md)


def _spread(shape, gen):
    """fp32 values of both signs with magnitudes over four decades (1e-2 .. 1e2 times a normal deviate)"""
    return (torch.randn(shape, generator=gen) * 10.0 ** (4.0 * torch.rand(shape, generator=gen) - 2.0)).float()


def _hold(group, what, got, want64, bound):
    """got within `bound` (elementwise, float64) of want64; records the achieved share of the bound"""
    import errtable
    got = got.detach().double().cpu()
    want64, bound = want64.cpu(), bound.cpu()
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = (got - want64).abs()
    used = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    i = int(err.flatten().argmax())
    errtable.record(f"{group} {what}", got.numpy(), want64.numpy(), float(bound.flatten()[i]))
    ACHIEVED[group] = max(ACHIEVED.get(group, 0.0), used)
    print(f"[{group}] {what}: max|got - f64| = {float(err.max()):.3e}, bound there {float(bound.flatten()[i]):.3e}, worst share of the bound {used:.2e}"
          f" (group so far {ACHIEVED[group]:.2e})")
    assert bool((err <= bound).all()), f"{what}: |got - f64| exceeds the bound: worst share {used:.3f}"


class _Arena:
    """Outputs of the given sizes (0 = absent) inside one canary-filled buffer: [gap | out0 | gap | out1 | ... | gap]."""

    def __init__(self, sizes):
        self.sizes, self.offs, off = list(sizes), [], GAP
        for s in self.sizes:
            self.offs.append(off)
            off += s + (GAP if s else 0)
        self.buf = torch.full((off,), CANARY, dtype=torch.float32, device=DEV)

    def out(self, i):
        return self.buf[self.offs[i]:self.offs[i] + self.sizes[i]] if self.sizes[i] else None

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.offs[i] if self.sizes[i] else 0

    def expected(self, values):
        """the buffer as it must look after the call: canary everywhere but `values[i]` in output i"""
        e = torch.full_like(self.buf, CANARY)
        for i, v in enumerate(values):
            if self.sizes[i]:
                e[self.offs[i]:self.offs[i] + self.sizes[i]] = v.reshape(-1)
        return e

    def untouched(self):
        return bool((self.buf == torch.full_like(self.buf, CANARY)).all())

    def wipe(self):
        self.buf.fill_(CANARY)


def _assert_arena(arena, values, what):
    want = arena.expected(values)
    if not torch.equal(arena.buf, want):
        bad = (arena.buf != want).nonzero().flatten()
        inside = torch.zeros_like(arena.buf, dtype=torch.bool)
        for o, s in zip(arena.offs, arena.sizes):
            inside[o:o + s] = True
        n_out = int((~inside[bad]).sum())
        raise AssertionError(f"{what}: {bad.numel()} floats differ from the fp32 definition, {n_out} of them outside the outputs (canary overwritten); "
                             f"first at {int(bad[0])}: got {float(arena.buf[bad[0]])!r}, want {float(want[bad[0]])!r}")


# ---- the weight-gradient finish ---------------------------------------------------------------------------------------------------------
def _wg_item(gen, S, N, K, extra, pad=0):
    """One table item: parts (S, N, ld), ld = K + extra + pad, extra = how many of (db, e1, e2) are present; padding columns 1e30."""
    cols, ld = K + extra, K + extra + pad
    parts = _spread((S, N, ld), gen)
    parts[..., cols:] = 1e30
    return dict(parts=parts.to(DEV), S=S, N=N, K=K, ld=ld, cols=cols, arena=_Arena([N * K] + [N if extra > i else 0 for i in range(3)]))


def _wg_call(items):
    """vmasr_wgrad_finish_multi with pointer arrays, as wgrad._launch passes them; -> the return code"""
    from vm_asr_amd import _lib
    arr = lambda f, dt: np.array([f(it) for it in items], dtype=dt)     # noqa: E731
    parts = arr(lambda it: it["parts"].data_ptr(), np.uint64)
    outs = [arr(lambda it, i=i: it["arena"].ptr(i), np.uint64) for i in range(4)]
    dims = [arr(lambda it, k=k: it[k], np.int32) for k in ("S", "N", "K", "ld")]
    with torch.cuda.device(torch.device(DEV)):
        return _lib.lib().vmasr_wgrad_finish_multi(parts.ctypes.data, *[o.ctypes.data for o in outs], *[d.ctypes.data for d in dims], len(items),
                                                   _lib.current_stream(torch.device(DEV)))


def _wg_definition(it):
    """fp32, slab after slab: the kernel's summation order"""
    s = torch.zeros_like(it["parts"][0])
    for j in range(it["S"]):
        s = s + it["parts"][j]
    K = it["K"]
    return [s[:, :K].contiguous()] + [s[:, K + i].contiguous() for i in range(it["cols"] - K)] + [None] * (3 - (it["cols"] - K))


def _wg_run_and_check(items, group):
    from vm_asr_amd import _lib
    assert _wg_call(items) == 0, _lib.lib().vmasr_last_error()
    torch.cuda.synchronize()
    first = [it["arena"].buf.clone() for it in items]
    for i, it in enumerate(items):
        what = f"item {i} of {len(items)} (S {it['S']}, N {it['N']}, K {it['K']}, cols {it['cols']}, ld {it['ld']})"
        _assert_arena(it["arena"], _wg_definition(it), what)
        N, K, cols = it["N"], it["K"], it["cols"]
        got = torch.cat([it["arena"].out(0).view(N, K)] + [it["arena"].out(1 + c).view(N, 1) for c in range(cols - K)], dim=1)
        p64 = it["parts"][..., :cols].double()
        _hold(group, what, got, p64.sum(0), it["S"] * U * p64.abs().sum(0))
    for it in items:
        it["arena"].wipe()
    assert _wg_call(items) == 0
    torch.cuda.synchronize()
    for i, (it, a) in enumerate(zip(items, first)):
        assert torch.equal(it["arena"].buf, a), f"item {i}: the second run differs from the first"


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_wgrad_finish_column_layouts(extra, pad):
    """dw only; dw + db; dw + db + e1; dw + db + e1 + e2 — each with ld == cols and with five 1e30 padding columns"""
    gen = torch.Generator().manual_seed(10 * extra + pad)
    _wg_run_and_check([_wg_item(gen, 4, 7, 5, extra, pad)], "wgrad layouts")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 4, 37])
def test_wgrad_finish_slab_counts(S):
    gen = torch.Generator().manual_seed(S)
    _wg_run_and_check([_wg_item(gen, S, 33, 9, 2, 5)], "wgrad slab counts")


# (N, K, extra, ld): around the launch's 64 * 256 = 16 384 threads — one element; exactly 16 384; 16 640 (a partial second sweep);
# 38 400 (three sweeps); and the shapes of the model: fc-like (32, 8) in ld 16, (256, 64) in ld 72, the deep core's (4 D, R) in ld 20
SIZES = [(1, 1, 0, 1), (256, 63, 1, 64), (256, 64, 1, 65), (512, 72, 3, 75), (32, 8, 1, 16), (256, 64, 1, 72), (256, 4, 3, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("N, K, extra, ld", SIZES)
def test_wgrad_finish_sizes_around_one_grid_sweep(N, K, extra, ld):
    gen = torch.Generator().manual_seed(N + K)
    _wg_run_and_check([_wg_item(gen, 4, N, K, extra, ld - K - extra)], "wgrad sizes")


@pytest.mark.gpu
def test_wgrad_finish_mixed_table_small_items_complete_large_item_swept():
    """The grid is sized by the largest item of the table: the 1 x 1 item must not be touched twice, the 512 x 75 one must be swept whole."""
    gen = torch.Generator().manual_seed(7)
    items = [_wg_item(gen, 3, 1, 1, 0), _wg_item(gen, 4, 512, 72, 3), _wg_item(gen, 5, 32, 8, 1, 7), _wg_item(gen, 2, 256, 64, 1, 7)]
    _wg_run_and_check(items, "wgrad mixed table")


def _wg_distinct(gen, i):
    """item i of a long table: S, N, K, layout and padding all depend on i, so a swapped or repeated table slot cannot pass"""
    return _wg_item(gen, 1 + i % 5, 1 + (7 * i) % 13, 1 + (3 * i) % 11, i % 4, 2 * (i % 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 39, 40, 41, 80, 81])
def test_wgrad_finish_item_counts_across_the_40_item_table(n):
    gen = torch.Generator().manual_seed(n)
    _wg_run_and_check([_wg_distinct(gen, i) for i in range(n)], "wgrad item counts")


@pytest.mark.gpu
def test_wgrad_finish_refuses_a_bad_item_before_any_launch():
    """S = 0 at index 44 of 46: the first table (items 0..39) must not have been launched when the call is refused."""
    from vm_asr_amd import _lib
    gen = torch.Generator().manual_seed(44)
    items = [_wg_distinct(gen, i) for i in range(46)]
    items[44]["S"] = 0
    assert _wg_call(items) == -1
    assert b"wgrad_finish_multi: bad item 44" in _lib.lib().vmasr_last_error()
    torch.cuda.synchronize()
    written = [i for i, it in enumerate(items) if not it["arena"].untouched()]
    assert not written, f"refused call wrote the outputs of items {written}"


# ---- LayerNorm's dgamma / dbeta reduction ------------------------------------------------------------------------------------------------
def _lpr(C):
    lpr = 1
    while lpr < 64 and lpr * 4 < C:
        lpr *= 2
    return lpr


def _ln_partials(gen, C, nblk, i=0):
    """The per-workgroup partials (nblk, 2, C) that vmasr_layer_norm_bwd leaves in its workspace for a (rows, C) call whose grid is
    `nblk` workgroups, and the dgamma / dbeta its own reduction writes for them."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    rpb = 256 // _lpr(C)
    rows = (nblk - 1) * rpb + 1 + (i % rpb)              # last workgroup partly filled
    assert lib.vmasr_layer_norm_bwd_blocks(rows, C) == nblk, (rows, C, nblk)
    x, gy = _spread((rows, C), gen).to(DEV), _spread((rows, C), gen).to(DEV)
    gamma = (1 + 0.1 * torch.randn(C, generator=gen)).to(DEV)
    mean = x.mean(1)
    rstd = ((x - mean[:, None]).square().mean(1) + 1e-5).rsqrt()
    dx = torch.empty_like(x)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = torch.empty(lib.vmasr_layer_norm_bwd_workspace(rows, C) // 4, device=DEV)
    assert ws.numel() == nblk * 2 * C
    _lib.call(lib.vmasr_layer_norm_bwd, x, gy, gamma, mean, rstd, dx, dg, db, ws, rows, C, _lib.F32, _lib.F32)
    return dict(part=ws.view(nblk, 2, C), nblk=nblk, C=C, dg=dg, db=db)


def _ln_item(p, i):
    """outputs for partials `p`; item i leaves dgamma (i % 3 == 1) or dbeta (i % 3 == 2) null"""
    C = p["C"]
    return dict(p, arena=_Arena([0 if i % 3 == 1 else C, 0 if i % 3 == 2 else C]))


def _ln_call(items):
    from vm_asr_amd import _lib
    arr = lambda f, dt: np.array([f(it) for it in items], dtype=dt)     # noqa: E731
    parts = arr(lambda it: it["part"].data_ptr(), np.uint64)
    dgs, dbs = arr(lambda it: it["arena"].ptr(0), np.uint64), arr(lambda it: it["arena"].ptr(1), np.uint64)
    nblk, Cs = arr(lambda it: it["nblk"], np.int32), arr(lambda it: it["C"], np.int32)
    with torch.cuda.device(torch.device(DEV)):
        return _lib.lib().vmasr_layer_norm_bwd_reduce_multi(parts.ctypes.data, dgs.ctypes.data, dbs.ctypes.data, nblk.ctypes.data, Cs.ctypes.data,
                                                            len(items), _lib.current_stream(torch.device(DEV)))


def _ln_run_and_check(items, group):
    from vm_asr_amd import _lib
    assert _ln_call(items) == 0, _lib.lib().vmasr_last_error()
    torch.cuda.synchronize()
    for i, it in enumerate(items):
        what = f"item {i} of {len(items)} (nblk {it['nblk']}, C {it['C']})"
        _assert_arena(it["arena"], [it["dg"], it["db"]], what)        # bit for bit the one-item kernel's result, canaries intact
        p64 = it["part"].double()
        for k, name in enumerate(("dgamma", "dbeta")):
            if it["arena"].sizes[k]:
                _hold(group, f"{what} {name}", it["arena"].out(k), p64[:, k].sum(0), it["nblk"] * U * p64[:, k].abs().sum(0))


LN_C = (1, 3, 4, 130, 1024)        # 130 > the 32 * 4 columns of one grid sweep: the column stride
LN_NBLK = (1, 63, 64, 65)          # around one 64-lane sweep over the partials


@pytest.fixture(scope="module")
def ln_pool():
    """193 distinct partials, computed once: item i has C = LN_C[i % 5] and nblk = LN_NBLK[(i // 5) % 4], its own data and row count"""
    gen = torch.Generator().manual_seed(193)
    return [_ln_partials(gen, LN_C[i % 5], LN_NBLK[(i // 5) % 4], i) for i in range(193)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 95, 96, 97, 193])
def test_layer_norm_reduce_item_counts_across_the_96_item_table(ln_pool, n):
    _ln_run_and_check([_ln_item(p, i) for i, p in enumerate(ln_pool[:n])], "ln reduce item counts")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 130])
def test_layer_norm_reduce_2048_partials(C):
    """the largest grid LayerNorm's backward launches (2 048 workgroups): 32 sweeps of the 64 lanes; next to a one-partial item"""
    gen = torch.Generator().manual_seed(C)
    items = [_ln_item(_ln_partials(gen, C, 2048), 0), _ln_item(_ln_partials(gen, 1024, 1), 0), _ln_item(_ln_partials(gen, C, 2048, 5), 1 + C % 2)]
    _ln_run_and_check(items, "ln reduce 2048 partials")


@pytest.mark.gpu
def test_layer_norm_reduce_refuses_a_bad_item_before_any_launch(ln_pool):
    """nblk = 0 at index 98 of 100: the first table (items 0..95) must not have been launched when the call is refused."""
    from vm_asr_amd import _lib
    items = [_ln_item(p, i) for i, p in enumerate(ln_pool[:100])]
    items[98]["nblk"] = 0
    assert _ln_call(items) == -1
    assert b"layer_norm_bwd_reduce_multi: bad item 98" in _lib.lib().vmasr_last_error()
    torch.cuda.synchronize()
    written = [i for i, it in enumerate(items) if not it["arena"].untouched()]
    assert not written, f"refused call wrote the outputs of items {written}"


# ---- the host queue (vm_asr_amd/wgrad.py) -----------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for lib.vmasr_wgrad_finish_multi: records each call's table, then runs the real entry point."""
    __name__ = "vmasr_wgrad_finish_multi"

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, parts, dws, dbs, e1s, e2s, Ss, Ns, Ks, lds, n, stream):
        from vm_asr_amd import wgrad
        rd = lambda p: [int(v) for v in (ctypes.c_int32 * n).from_address(p)]       # noqa: E731
        self.calls.append(dict(n=n, S=rd(Ss), N=rd(Ns), K=rd(Ks), ld=rd(lds), queued=len(wgrad._Q.items)))
        return self.real(parts, dws, dbs, e1s, e2s, Ss, Ns, Ks, lds, n, stream)


@pytest.fixture
def spy(monkeypatch):
    from vm_asr_amd import _lib
    lib = _lib.lib()
    s = _Spy(lib.vmasr_wgrad_finish_multi)
    monkeypatch.setattr(lib, "vmasr_wgrad_finish_multi", s)
    return s


TAPE = []      # (weight, gy, x, spy calls before, spy calls after) per backward of _Lin, when a test asks for it
_SPY = [None]


class _Lin(torch.autograd.Function):
    """y = x W^T + b with the weight-gradient protocol of mlp.py: note_use in forward, weight_grad_finished(..., fresh=...) in backward"""
    @staticmethod
    def forward(ctx, x, weight, bias):
        from vm_asr_amd import layernorm
        ctx.save_for_backward(x, weight)
        if any(ctx.needs_input_grad[1:3]):
            layernorm.note_use(weight, bias)
        ctx.params = (weight, bias)
        return torch.addmm(bias, x, weight.t())

    @staticmethod
    def backward(ctx, gy):
        from vm_asr_amd import layernorm, wgrad
        x, w = ctx.saved_tensors
        rows, K = x.shape
        gy2 = gy.contiguous()
        x_aug = torch.cat([x, torch.ones(rows, 1, device=x.device), torch.zeros(rows, 3, device=x.device)], dim=1)      # [x | 1 | 0 0 0]
        before = len(_SPY[0].calls) if _SPY[0] else 0
        dw, db = wgrad.weight_grad_finished(gy2, x_aug, K, ctx.params[0], ctx.params[1], fresh=layernorm.fresh(*ctx.params))
        TAPE.append((ctx.params[0], gy2.detach().clone(), x.detach(), before, len(_SPY[0].calls) if _SPY[0] else 0))
        return gy2 @ w, dw, db


class Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


WIDTHS = (8, 16, 32, 64)


def _chain(n_layers, seed=0):
    gen = torch.Generator().manual_seed(seed)
    ws, bs = [], []
    for i in range(n_layers):
        k, n = WIDTHS[i % 4], WIDTHS[(i + 1) % 4]
        ws.append((torch.randn(n, k, generator=gen) / k ** 0.5).to(DEV).requires_grad_())
        bs.append((0.1 * torch.randn(n, generator=gen)).to(DEV).requires_grad_())
    x = torch.randn(512, WIDTHS[0], generator=gen).to(DEV)
    gy = _spread((512, WIDTHS[n_layers % 4]), gen).to(DEV)
    return ws, bs, x, gy


def _chain_backward(ws, bs, x, gy, defer, keep_grads=False):
    from vm_asr_amd import layernorm
    if not keep_grads:
        for p in ws + bs:
            p.grad = None
    del TAPE[:]
    with layernorm.deferred(defer):
        h = x
        for w, b in zip(ws, bs):
            h = _Lin.apply(h, w, b)
        h.backward(gy)
    torch.cuda.synchronize()
    assert not layernorm.DEFER_REDUCE
    return [p.grad.clone() for p in ws + bs]


def _hold_tape(group, ws, bs, grads):
    """every layer's dW, db against gy^T [x | 1] in float64, from the operands its backward saw"""
    n = len(ws)
    by_weight = {id(t[0]): t for t in TAPE}
    for i, w in enumerate(ws):
        _, gy, x = by_weight[id(w)][:3]
        rows = x.shape[0]
        g64, x64 = gy.double(), x.double()
        _hold(group, f"layer {i} dW", grads[i], g64.t() @ x64, rows * U * (g64.abs().t() @ x64.abs()))
        _hold(group, f"layer {i} db", grads[n + i], g64.sum(0), rows * U * g64.abs().sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", [25, 45])
def test_queue_deferred_equals_immediate_over_a_chain(spy, n_layers):
    """25 layers: one item each (dW and db travel together), one launch.  45 layers: more than one 40-item table, still one call from Python."""
    from vm_asr_amd import layernorm, wgrad
    _SPY[0] = spy
    try:
        ws, bs, x, gy = _chain(n_layers)
        ref = _chain_backward(ws, bs, x, gy, False)
        assert [c["n"] for c in spy.calls] == [1] * n_layers
        _hold_tape("queue chain immediate", ws, bs, ref)
        del spy.calls[:]
        got = _chain_backward(ws, bs, x, gy, True)
        assert wgrad._Q.items == [] and layernorm._pending == []
        assert [c["n"] for c in spy.calls] == [n_layers], [c["n"] for c in spy.calls]
        assert all(t[3] == t[4] == 0 for t in TAPE), "a deferred item was launched during the backward"
        call = spy.calls[0]                      # in backward order: last layer first
        want = [(1, w.shape[0], w.shape[1], w.shape[1] + 4) for w in reversed(ws)]
        assert list(zip(call["S"], call["N"], call["K"], call["ld"])) == want
        for i, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, b), f"gradient {i} of {2 * n_layers}: deferred differs from immediate"
        _hold_tape("queue chain deferred", ws, bs, got)
        assert all(p.grad.is_contiguous() for p in ws + bs)
    finally:
        _SPY[0] = None


@pytest.mark.gpu
def test_queue_split_k_on_and_off(spy):
    """rows = 4 chunks: four slabs.  One row more: rows % S != 0, one plain GEMM (S = 1).  Both against float64."""
    from vm_asr_amd import linear, wgrad
    chunk = linear._SPLITK_CHUNK
    for rows, want_S in ((4 * chunk, 4), (4 * chunk + 1, 1)):
        assert linear.splitk_plan(rows, 32, 16) == 4
        gen = torch.Generator().manual_seed(rows)
        gy, x = _spread((rows, 32), gen).to(DEV), torch.randn(rows, 12, generator=gen).to(DEV)
        x_aug = torch.cat([x, torch.ones(rows, 1, device=DEV), torch.zeros(rows, 3, device=DEV)], dim=1)
        del spy.calls[:]
        dw, db = wgrad.weight_grad_finished(gy, x_aug, 12)
        torch.cuda.synchronize()
        assert [(c["n"], c["S"], c["N"], c["K"], c["ld"]) for c in spy.calls] == [(1, [want_S], [32], [12], [16])]
        g64, x64 = gy.double(), x.double()
        _hold("queue split-K", f"rows {rows} S {want_S} dW", dw, g64.t() @ x64, rows * U * (g64.abs().t() @ x64.abs()))
        _hold("queue split-K", f"rows {rows} S {want_S} db", db, g64.sum(0), rows * U * g64.abs().sum(0))


@pytest.mark.gpu
def test_linear_weight_grad_splits_with_a_remainder():
    """linear.weight_grad(splits = S) with rows = S * chunk + 3: the three rows past the slabs are a GEMM of their own"""
    from vm_asr_amd import linear
    S, chunk = 4, 500
    rows = S * chunk + 3
    gen = torch.Generator().manual_seed(3)
    gy, x = _spread((rows, 24), gen).to(DEV), _spread((rows, 10), gen).to(DEV)
    dw = linear.weight_grad(gy, x, splits=S)
    g64, x64 = gy.double(), x.double()
    _hold("queue split-K", "weight_grad remainder dW", dw, g64.t() @ x64, rows * U * (g64.abs().t() @ x64.abs()))
    # the remainder matters: without its rows the result is outside the bound somewhere
    short = g64[:S * chunk].t() @ x64[:S * chunk]
    assert bool(((short - g64.t() @ x64).abs() > rows * U * (g64.abs().t() @ x64.abs())).any())


def _two_contributions(group, param_grad, taped, rows):
    (_, g1, x1), (_, g2, x2) = [t[:3] for t in taped]
    g1, x1, g2, x2 = g1.double(), x1.double(), g2.double(), x2.double()
    want = g1.t() @ x1 + g2.t() @ x2
    _hold(group, "dW of two contributions", param_grad, want, (rows + 1) * U * (g1.abs().t() @ x1.abs() + g2.abs().t() @ x2.abs()))


@pytest.mark.gpu
def test_queue_finishes_at_once_for_a_parameter_used_twice(spy):
    from vm_asr_amd import layernorm, wgrad
    _SPY[0] = spy
    try:
        gen = torch.Generator().manual_seed(5)
        w = (torch.randn(16, 16, generator=gen) / 4).to(DEV).requires_grad_()
        b = (0.1 * torch.randn(16, generator=gen)).to(DEV).requires_grad_()
        x, gy = torch.randn(512, 16, generator=gen).to(DEV), _spread((512, 16), gen).to(DEV)
        del TAPE[:]
        with layernorm.deferred(True):
            _Lin.apply(_Lin.apply(x, w, b), w, b).backward(gy)
            assert wgrad._Q.items == []
        torch.cuda.synchronize()
        assert [(c["n"], c["queued"]) for c in spy.calls] == [(1, 0), (1, 0)]
        assert [(t[3], t[4]) for t in TAPE] == [(0, 1), (1, 2)], "the one-item calls must happen DURING the backward"
        _two_contributions("queue immediate fallback", w.grad, TAPE, 512)
    finally:
        _SPY[0] = None


@pytest.mark.gpu
def test_queue_finishes_at_once_for_a_parameter_that_holds_a_grad(spy):
    from vm_asr_amd import wgrad
    _SPY[0] = spy
    try:
        ws, bs, x, gy = _chain(1, seed=6)
        _chain_backward(ws, bs, x, gy, False)
        first = list(TAPE)
        del spy.calls[:]
        _chain_backward(ws, bs, 2 * x, gy, True, keep_grads=True)        # .grad is there: accumulate in place, finish at once
        assert wgrad._Q.items == []
        assert [(c["n"], c["queued"]) for c in spy.calls] == [(1, 0)] and [(t[3], t[4]) for t in TAPE] == [(0, 1)]
        _two_contributions("queue immediate fallback", ws[0].grad, first + list(TAPE), 512)
    finally:
        _SPY[0] = None


@pytest.mark.gpu
def test_queue_fills_a_grad_that_autograd_cloned_instead_of_adopting():
    """A tensor hook that keeps the gradient it is handed holds a second reference, so autograd clones the (still unfinished) tensor
    into .grad: the flush has to copy the finished values over, and the tensor the hook kept is finished too."""
    ws, bs, x, gy = _chain(3, seed=8)
    ref = _chain_backward(ws, bs, x, gy, False)
    kept = []
    h = ws[1].register_hook(lambda g: kept.append(g))
    try:
        got = _chain_backward(ws, bs, x, gy, True)
    finally:
        h.remove()
    assert len(kept) == 1 and ws[1].grad.data_ptr() != kept[0].data_ptr(), "autograd was expected to clone here"
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(a, b), f"gradient {i}: deferred differs from immediate"
    assert torch.equal(kept[0], ref[1])


class _Cols(torch.autograd.Function):
    """Four parameters of the deep SS2D core's shapes whose gradients are dW and columns K, K + 1, K + 2 of given slabs (finish_slabs)."""
    @staticmethod
    def forward(ctx, x, parts, wdt, dtb, alog, ds):
        from vm_asr_amd import layernorm
        ps = (wdt, dtb, alog, ds)
        layernorm.note_use(*ps)
        ctx.params, ctx.parts = ps, parts
        return x.clone()

    @staticmethod
    def backward(ctx, gy):
        from vm_asr_amd import layernorm, wgrad
        S, N, ld = ctx.parts.shape
        dw = torch.empty((N, 4), dtype=torch.float32, device=gy.device)
        c4, c5, c6 = (torch.empty(N, dtype=torch.float32, device=gy.device) for _ in range(3))
        wgrad.finish_slabs(ctx.parts, 4, (dw, c4, c5, c6), ctx.params, layernorm.fresh(*ctx.params))
        return (gy, None) + tuple(t.view(p.shape) for t, p in zip((dw, c4, c5, c6), ctx.params))


@pytest.mark.gpu
@pytest.mark.parametrize("hooked", [None, 2, 3])
def test_queue_extra_columns_through_finish_slabs(spy, hooked):
    """parts (S, 4 D, 20), K = 4: dW_dt (4, D, 4), d dt_bias (4, D), dA_log (4 D, 1), dD (4 D) — parameter shapes that differ from the flat
    outputs; deferred against immediate and against the definition; hooked: the parameter whose gradient autograd has to clone."""
    from vm_asr_amd import layernorm, wgrad
    D, S = 16, 6
    gen = torch.Generator().manual_seed(20)
    parts = _spread((S, 4 * D, 20), gen)
    parts[..., 7:] = 1e30
    parts = parts.to(DEV)
    params = [torch.zeros(s, device=DEV).requires_grad_() for s in ((4, D, 4), (4, D), (4 * D, 1), (4 * D,))]
    x = torch.randn(3, 5, device=DEV, requires_grad=True)
    s = torch.zeros_like(parts[0])
    for j in range(S):
        s = s + parts[j]
    want = [s[:, :4].reshape(4, D, 4), s[:, 4].reshape(4, D), s[:, 5].reshape(4 * D, 1), s[:, 6].reshape(4 * D)]

    def run(defer):
        for p in params:
            p.grad = None
        with layernorm.deferred(defer):
            _Cols.apply(x, parts, *params).sum().backward()
            assert wgrad._Q.items == []
        torch.cuda.synchronize()
        return [p.grad.clone() for p in params]
    ref = run(False)
    assert [(c["n"], c["S"], c["N"], c["K"], c["ld"]) for c in spy.calls] == [(1, [S], [4 * D], [4], [20])]
    kept = []
    h = params[hooked].register_hook(lambda g: kept.append(g)) if hooked is not None else None
    try:
        got = run(True)
    finally:
        if h is not None:
            h.remove()
    assert len(spy.calls) == 2 and spy.calls[1]["queued"] == 0
    if hooked is not None:
        assert params[hooked].grad.data_ptr() != kept[0].data_ptr(), "autograd was expected to clone here"
        assert torch.equal(kept[0], want[hooked])
    for i, (a, b, c) in enumerate(zip(ref, got, want)):
        assert a.shape == c.shape and torch.equal(a, c), f"output {i}: immediate differs from the definition"
        assert torch.equal(b, c), f"output {i}: deferred differs from the definition"


@pytest.mark.gpu
def test_queue_survives_an_aborted_backward():
    """A backward that raises after an item was queued never reaches the end-of-pass callback: leaving the `deferred` scope drops the
    item, and the next deferred backward is complete and correct."""
    from vm_asr_amd import layernorm, wgrad
    ws, bs, x, gy = _chain(2, seed=9)
    ref = _chain_backward(ws, bs, x, gy, False)
    for p in ws + bs:
        p.grad = None
    xg = x.clone().requires_grad_()
    queued = []
    with pytest.raises(RuntimeError, match="boom"):
        with layernorm.deferred(True):
            y = _Lin.apply(_Lin.apply(Boom.apply(xg), ws[0], bs[0]), ws[1], bs[1])
            try:
                y.backward(gy)
            finally:
                queued.append(len(wgrad._Q.items))         # (still inside the scope)
    assert queued == [2], "both layers' backward must have queued before Boom raised"
    assert wgrad._Q.items == [] and layernorm._pending == [] and not layernorm.DEFER_REDUCE
    got = _chain_backward(ws, bs, x, gy, True)
    assert wgrad._Q.items == []
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(a, b), f"gradient {i} after an aborted pass"


# ---- the real operators --------------------------------------------------------------------------------------------------------------------
def _deferred_vs_immediate(params, forward):
    from vm_asr_amd import layernorm, wgrad

    def run(defer):
        for p in params:
            p.grad = None
        with layernorm.deferred(defer):
            forward().backward()
            assert wgrad._Q.items == [] and layernorm._pending == []
        torch.cuda.synchronize()
        assert all(p.grad is not None for p in params)
        return [p.grad.clone() for p in params]
    return run(False), run(True), run(False)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [8, 32])
def test_fused_blocks_deferred_gradients_equal_immediate_bit_for_bit(spy, d):
    """Three blocks of LayerNorm -> in_proj -> gate -> out_proj + residual -> fused Mlp + residual in one graph under bf16 autocast: every
    parameter gradient of the deferred pass (one finish launch, one LayerNorm reduce launch) equals the immediate pass' bit for bit."""
    from vm_asr_amd import inproj, mlp as M, outproj
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.linear import Linear
    from vm_asr_amd.vmamba import Mlp
    torch.manual_seed(d)
    blocks = [dict(norm=LayerNorm(d).to(DEV), inp=Linear(d, 4 * d, bias=False).to(DEV), out=Linear(2 * d, d, bias=False).to(DEV),
                   norm2=LayerNorm(d).to(DEV), mlp=Mlp(d, 4 * d).to(DEV)) for _ in range(3)]
    params = [p for b in blocks for m in b.values() for p in m.parameters()]
    with torch.no_grad():
        for p in params:
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    shape = (2, 16, 16) if d == 8 else (2, 8, 16)          # the smallest shapes of tests/test_mlp.py at these widths
    x = torch.randn(*shape, d, device=DEV)
    gy = torch.randn(*shape, d, device=DEV)

    def forward():
        h = x.clone().requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for b in blocks:
                assert inproj.supported(h, b["norm"], b["inp"])
                xT, sz = inproj.fused_in_proj(h, b["norm"], b["inp"])
                g = xT.permute(0, 2, 3, 1).contiguous() * sz
                assert outproj.supported(g, b["out"], h) and M.supported(h, b["norm2"], b["mlp"])
                h = outproj.fused_out_proj_residual(g, b["out"], h)
                h = M.fused_mlp_residual(h, b["norm2"], b["mlp"])
        return (h.float() * gy).sum()
    ref, got, again = _deferred_vs_immediate(params, forward)
    ns = [c["n"] for c in spy.calls]
    assert ns == [1] * 12 + [12] + [1] * 12, ns                    # per block: in_proj, out_proj, fc1, fc2
    for i, (a, b, c) in enumerate(zip(ref, got, again)):
        assert torch.equal(a, c), f"parameter {i} {tuple(a.shape)}: two immediate passes differ"
        assert torch.equal(a, b), f"parameter {i} {tuple(a.shape)}: deferred differs from immediate by {(a - b).abs().max().item():.3e}"


@pytest.mark.gpu
def test_deep_core_deferred_gradients_equal_immediate_bit_for_bit(spy):
    """Three deep SS2D cores in one graph at the smallest shape of tests/test_ss2d_deep.py: two items each (dW_x; dW_dt with its three
    columns), one finish launch of six."""
    from test_ss2d_deep import _params
    from vm_asr_amd.ss2d_deep import ss2d_deep, supported
    B, D, H, W, R = 1, 64, 8, 32, 8
    assert supported(1, R, D, H, W)
    cores = [[p.to(DEV).requires_grad_() for p in _params(D, R, 30 + k)] for k in range(3)]
    params = [p for c in cores for p in c]
    gen = torch.Generator().manual_seed(31)
    x, gy = torch.randn(B, D, H, W, generator=gen).to(DEV), torch.randn(B, D, H * W, generator=gen).to(DEV)

    def forward():
        h = x.clone().requires_grad_()
        for c in cores:
            h = ss2d_deep(h, *c).view(B, D, H, W) * 0.5
        return (h.view(B, D, H * W) * gy).sum()
    ref, got, again = _deferred_vs_immediate(params, forward)
    ns = [c["n"] for c in spy.calls]
    assert ns == [1] * 6 + [6] + [1] * 6, ns
    for i, (a, b, c) in enumerate(zip(ref, got, again)):
        assert torch.equal(a, c), f"parameter {i} {tuple(a.shape)}: two immediate passes differ"
        assert torch.equal(a, b), f"parameter {i} {tuple(a.shape)}: deferred differs from immediate by {(a - b).abs().max().item():.3e}"
