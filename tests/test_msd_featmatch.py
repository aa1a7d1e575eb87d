"""The scale discriminator's generator pass with its feature-matching loss, on the host (no GPU needed): forward_generator on CPU tensors
is forward_single + the reference's loop bit for bit, the VMASR_MSD_FEAT switch, the four new symbols of include/vmasr_hip.h with the
argument lists the bindings use, the launchers' argument checks, and the launch predicate against a Python restatement of its bounds."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vmasr_hip.h")


def _small_msd():
    from vm_asr_amd.msd import MultiScaleDiscriminator
    torch.manual_seed(31)
    return MultiScaleDiscriminator(hidden=16).eval()


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_forward_generator_on_cpu_is_the_composed_route_bitwise(mode, monkeypatch):
    monkeypatch.setenv("VMASR_MSD_FEAT", mode)
    D = _small_msd()
    real, x = 0.3 * torch.randn(2, 1, 1201), (0.3 * torch.randn(2, 1, 1201)).requires_grad_()
    with torch.no_grad():
        _, f_real = D.forward_single(real, detach_weights=True)
    scores, loss = D.forward_generator(x, f_real)
    (loss + sum((s ** 2).mean() for s in scores)).backward()
    got_dx, x.grad = x.grad.clone(), None
    assert all(p.grad is None for p in D.parameters())
    ref_scores, fmaps = D.forward_single(x, detach_weights=True)
    want, n = 0, 0
    for dr, dg in zip(f_real, fmaps):
        for rl, gl in zip(dr, dg):
            n += 1
            want = want + torch.mean(torch.abs(rl - gl))
    want = want / n
    (want + sum((s ** 2).mean() for s in ref_scores)).backward()
    assert n == 24 and loss.dim() == 0 and torch.equal(loss, want)
    assert len(scores) == 3 and all(torch.equal(a, b) for a, b in zip(scores, ref_scores))
    assert torch.equal(got_dx, x.grad)


def test_forward_generator_keeps_the_power_iteration_schedule():
    """Training mode: one power iteration per weight, as forward_single spends (the same u / v afterwards)."""
    import copy
    A = _small_msd().train()
    B = copy.deepcopy(A)
    real, x = 0.3 * torch.randn(1, 1, 700), 0.3 * torch.randn(1, 1, 700)
    with torch.no_grad():
        _, f_real = A.forward_single(real, detach_weights=True)
        B.forward_single(real, detach_weights=True)
        A.forward_generator(x, f_real)
        B.forward_single(x, detach_weights=True)
    sa, sb = A.state_dict(), B.state_dict()
    assert sa.keys() == sb.keys() and any(k.endswith("_u") for k in sa)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_msd_feat_switch_is_declared(monkeypatch):
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_MSD_FEAT"]
    assert k.default in ("hip", "torch") and k.values == ("hip", "torch") and k.kind == "choice" and k.reader == "python:msd"
    monkeypatch.delenv("VMASR_MSD_FEAT", raising=False)
    assert knobs.get("VMASR_MSD_FEAT") == k.default
    for v in k.values:
        monkeypatch.setenv("VMASR_MSD_FEAT", v)
        assert knobs.get("VMASR_MSD_FEAT") == v
    monkeypatch.setenv("VMASR_MSD_FEAT", "fused")
    with pytest.raises(ValueError, match="VMASR_MSD_FEAT"):
        knobs.get("VMASR_MSD_FEAT")


_C2CT = {"const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "double *": ctypes.c_void_p, "vmasr_stream_t": ctypes.c_void_p,
         "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_RET = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}


def _declaration(name):
    """(return type, [parameter types]) of `name` as include/vmasr_hip.h declares it."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/vmasr_hip.h"
    params = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        ctype = p[:p.rindex("*") + 1] if "*" in p else p.rsplit(" ", 1)[0]
        params.append(" ".join(ctype.replace("*", " *").split()))
    return m.group(1), params


@pytest.mark.parametrize("name", ["vmasr_stem1d_fm_supported_launch", "vmasr_stem1d_fm_workspace", "vmasr_stem1d_fm_fwd", "vmasr_stem1d_fm_bwd"])
def test_new_symbols_are_declared_exported_and_prototyped_alike(name):
    from vm_asr_amd import _lib
    ret, params = _declaration(name)
    assert hasattr(_lib.lib(), name), f"{name} declared but not exported"
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is _RET[ret]
    assert list(argtypes) == [_C2CT[p] for p in params], (name, params)


def _admits(Cout, k, stride, pad, B, L):
    """The bounds include/vmasr_hip.h states for the stem, restated."""
    return (stride == 1 and 1 <= k <= 32 and 0 <= pad < k and 1 <= Cout <= 65536 and 1 <= B <= 65535
            and max(1, k - 2 * pad) <= L <= 1 << 28)


def test_fm_predicate_is_the_stems_on_both_sides_of_each_bound():
    from vm_asr_amd import _lib, msd_ops
    lib = _lib.lib()
    base = dict(Cout=128, k=15, stride=1, pad=7, B=4, L=1000)
    edges = {"stride": (0, 1, 2), "k": (0, 1, 32, 33), "pad": (-1, 0, 14, 15), "Cout": (0, 1, 65536, 65537), "B": (0, 1, 65535, 65536),
             "L": (0, 1, (1 << 28), (1 << 28) + 1)}
    cases = [dict(base, **{name: v}) for name, vs in edges.items() for v in vs]
    cases += [dict(base, pad=0, L=14), dict(base, pad=0, L=15), dict(base, k=4, pad=0, L=3), dict(base, k=4, pad=0, L=4), dict(base, L=1)]
    seen = set()
    for c in cases:
        args = (c["Cout"], c["k"], c["stride"], c["pad"], c["B"], c["L"])
        want = _admits(*args)
        seen.add(want)
        assert bool(lib.vmasr_stem1d_supported_launch(*args)) == want, args
        assert bool(lib.vmasr_stem1d_fm_supported_launch(*args)) == want, args
        assert msd_ops.stem1d_fm_supported_launch(*args) == want, args
        assert (lib.vmasr_stem1d_fm_workspace(*args) > 0) == want, args
    assert seen == {True, False}
    tile, cg = msd_ops.stem1d_time_tile(), msd_ops.stem1d_channel_group()
    # one fp64 slot per workgroup of the forward's grid
    assert lib.vmasr_stem1d_fm_workspace(128, 15, 1, 7, 4, 122640) == 8 * 4 * -(-128 // cg) * -(-122640 // tile)
    assert lib.vmasr_stem1d_fm_workspace(cg + 1, 15, 1, 7, 1, tile + 1) == 8 * 2 * 2


def test_fm_launchers_reject_bad_arguments():
    """Refused shapes, null pointers and a short workspace: the invalid-argument code (-1) before anything is launched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused first
    fwd, bwd = lib.vmasr_stem1d_fm_fwd, lib.vmasr_stem1d_fm_bwd
    good = (2, 128, 100, 15, 1, 7)
    for geom in ((2, 128, 100, 15, 2, 7), (2, 128, 100, 33, 1, 7), (2, 128, 100, 15, 1, 15), (2, 0, 100, 15, 1, 7), (0, 128, 100, 15, 1, 7),
                 (65536, 128, 100, 15, 1, 7), (2, 128, 14, 15, 1, 0), (2, 128, (1 << 28) + 1, 15, 1, 7)):
        assert fwd(p, p, p, p, p, p, 1 << 40, *geom, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
        assert bwd(p, p, p, p, p, p, 0.5, p, *geom, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
    for i in (0, 1, 3, 4):                                                            # x, w, y_real, y
        args = [p] * 6
        args[i] = None
        assert fwd(*args, 1 << 40, *good, None) == -1
        assert b"null" in lib.vmasr_last_error()
    assert fwd(p, p, p, p, p, None, 1 << 40, *good, None) == -1                       # no workspace
    assert b"workspace" in lib.vmasr_last_error()
    assert fwd(p, p, p, p, p, p, lib.vmasr_stem1d_fm_workspace(128, 15, 1, 7, 2, 100) - 1, *good, None) == -1
    assert b"workspace" in lib.vmasr_last_error()
    for i in (1, 2, 4, 7):                                                            # x, w, y_real, dx
        args = [p, p, p, p, p, p, 0.5, p]
        args[i] = None
        assert bwd(*args, *good, None) == -1
        assert b"null" in lib.vmasr_last_error()
    assert bwd(None, p, p, p, p, None, 0.5, p, *good, None) == -1                     # neither gradient
    assert b"null" in lib.vmasr_last_error()
