"""The scale discriminator's dense tail on the host (no GPU needed): the C ABI of csrc/dconv1d.hip and its bindings, the VMASR_MSD_TAIL
switch, the unchanged torch path of dense_conv1d for CPU tensors, the admitted-shape predicate and the launchers' argument checks, and
what the GPU test's case list reaches."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import msd_tail_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("supported", "supported_launch", "fwd", "dgrad", "wgrad", "wgrad_workspace", "fwd_workspace", "dgrad_workspace", "fwd_slabs",
                "pos_tile", "m_tile", "k_chunk", "max_taps")


def test_header_declares_the_entry_points_and_the_bindings_exist():
    from vm_asr_amd import _lib, msd, msd_ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vmasr_hip.h")).read(), flags=re.S)
    lib = _lib.lib()
    for n in ENTRY_POINTS:
        assert re.search(rf"\bvmasr_dconv1d_{n}\s*\(", src), n
        assert f"vmasr_dconv1d_{n}" in _lib.SYMBOLS and hasattr(lib, f"vmasr_dconv1d_{n}"), n
    for n in ("dconv1d_supported", "dconv1d_supported_launch", "dconv1d_fwd", "dconv1d_dgrad", "dconv1d_wgrad", "dconv1d_fwd_slabs", "dconv1d_tiles"):
        assert callable(getattr(msd_ops, n)), n
    assert callable(msd.dense_conv1d) and "dense_conv1d" in msd.__all__ and issubclass(msd._DConv1dFn, torch.autograd.Function)
    names = [lib.vmasr_prof_name(k) for k in range(_lib.K_COUNT)]
    assert all(n in names for n in (b"dconv1d_fwd", b"dconv1d_dgrad", b"dconv1d_reduce", b"dconv1d_wgrad", b"dconv1d_wgrad_reduce"))
    assert len(set(names)) == _lib.K_COUNT and b"" not in names and lib.vmasr_prof_name(_lib.K_COUNT) == b""


def test_msd_tail_switch_is_declared(monkeypatch):
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_MSD_TAIL"]
    # the default is the measurement's (profiles/msd_tail.md): the library route, faster on the 8h -> 8h layer
    assert k.default == "torch" and k.values == ("hip", "torch") and k.kind == "choice" and k.reader == "python:msd"
    monkeypatch.delenv("VMASR_MSD_TAIL", raising=False)
    assert knobs.get("VMASR_MSD_TAIL") == "torch"
    for v in k.values:
        monkeypatch.setenv("VMASR_MSD_TAIL", v)
        assert knobs.get("VMASR_MSD_TAIL") == v
    monkeypatch.setenv("VMASR_MSD_TAIL", "miopen")
    with pytest.raises(ValueError, match="VMASR_MSD_TAIL"):
        knobs.get("VMASR_MSD_TAIL")


@pytest.mark.parametrize("mode", ["hip", "torch"])
@pytest.mark.parametrize("act", [True, False])
def test_dense_conv1d_on_cpu_is_torch_and_twice_differentiable(mode, act, monkeypatch):
    """CPU tensors: bit-equal to F.conv1d (+ F.gelu) whatever the switch says, gradients included, and a double backward runs (the
    gradient penalty's path)."""
    from vm_asr_amd.msd import dense_conv1d
    monkeypatch.setenv("VMASR_MSD_TAIL", mode)
    g = torch.Generator().manual_seed(11)
    x, w, b = torch.randn(2, 6, 19, generator=g), torch.randn(4, 6, 5, generator=g) / 30 ** 0.5, torch.randn(4, generator=g)
    outs = []
    for fn in (lambda x, w, b: dense_conv1d(x, w, b, 1, 2, act), lambda x, w, b: F.gelu(F.conv1d(x, w, b, 1, 2)) if act else F.conv1d(x, w, b, 1, 2)):
        xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
        y = fn(xr, wr, br)
        gx, = torch.autograd.grad((y ** 2).sum(), xr, create_graph=True)
        (gx ** 2).sum().backward()
        outs.append((y.detach(), gx.detach(), xr.grad, wr.grad, br.grad))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert outs[0][3].abs().max() > 0
    y = dense_conv1d(x, w, None, 2, 1, act)                                  # stride 2: torch's operator as well
    assert torch.equal(y, F.gelu(F.conv1d(x, w, None, 2, 1)) if act else F.conv1d(x, w, None, 2, 1))


def test_dconv1d_predicates():
    from vm_asr_amd import _lib, msd_ops
    lib = _lib.lib()
    q, ql = msd_ops.dconv1d_supported, msd_ops.dconv1d_supported_launch
    kmax = msd_ops.dconv1d_tiles()[3]
    assert kmax >= 5
    assert q(1024, 1024, 1, 5, 1) and q(1024, 1, 1, 3, 1) and q(1, 1, 1, 1, 1) and q(65536, 65536, 1, kmax, 1)
    assert not q(1024, 1024, 1, 5, 2) and not q(1024, 1024, 2, 5, 1) and not q(1024, 1024, 1, kmax + 1, 1) and not q(1024, 1024, 1, 0, 1)
    assert not q(0, 8, 1, 5, 1) and not q(8, 0, 1, 5, 1) and not q(65537, 8, 1, 5, 1) and not q(8, 65537, 1, 5, 1) and not q(8, 8, 0, 5, 1)
    assert ql(1024, 1024, 1, 5, 1, 2, 8, 120) and ql(1024, 1, 1, 3, 1, 1, 8, 30) and ql(1, 1, 1, 1, 1, 0, 1, 1)
    assert ql(8, 8, 1, 5, 1, 4, 65535, 1 << 28) == (65535 * (((1 << 28) + 4 + 31) // 32) <= 1 << 30) and ql(8, 8, 1, 5, 1, 4, 2, 1 << 28)
    assert not ql(1024, 1024, 1, 5, 2, 2, 8, 120) and not ql(1024, 1024, 2, 5, 1, 2, 8, 120)                 # stride 2, groups 2
    assert not ql(1024, 1024, 1, 5, 1, 5, 8, 120) and not ql(1024, 1024, 1, 5, 1, -1, 8, 120)                # pad = k, pad < 0
    assert not ql(8, 8, 1, 5, 1, 2, 0, 120) and not ql(8, 8, 1, 5, 1, 2, 65536, 120)
    assert not ql(8, 8, 1, 5, 1, 0, 2, 4) and ql(8, 8, 1, 5, 1, 0, 2, 5) and not ql(8, 8, 1, 5, 1, 2, 2, 0)  # L < k - 2 pad: no output
    assert not ql(8, 8, 1, 5, 1, 2, 2, (1 << 28) + 1)
    for query in (lib.vmasr_dconv1d_fwd_workspace, lib.vmasr_dconv1d_dgrad_workspace, lib.vmasr_dconv1d_wgrad_workspace, lib.vmasr_dconv1d_fwd_slabs):
        assert query(1024, 1024, 1, 5, 2, 2, 8, 120) == 0 and query(1024, 1024, 2, 5, 1, 2, 8, 120) == 0 and query(8, 8, 1, 5, 1, 5, 2, 9) == 0
    # few output tiles: K slabs with a workspace of S (B, C, L) partials; many tiles: one slab and none
    S = msd_ops.dconv1d_fwd_slabs(1024, 1024, 1, 5, 1, 2, 4, 30)
    assert S > 1 and lib.vmasr_dconv1d_fwd_workspace(1024, 1024, 1, 5, 1, 2, 4, 30) == 4 * S * 4 * 1024 * 30
    assert msd_ops.dconv1d_fwd_slabs(64, 64, 1, 5, 1, 2, 64, 1 << 16) == 1 and lib.vmasr_dconv1d_fwd_workspace(64, 64, 1, 5, 1, 2, 64, 1 << 16) == 0
    assert lib.vmasr_dconv1d_wgrad_workspace(1024, 1024, 1, 5, 1, 2, 8, 120) == 0          # 16 x 32 (o, c) tiles own their whole K
    assert lib.vmasr_dconv1d_wgrad_workspace(8, 8, 1, 5, 1, 2, 8, 120) % (4 * (8 * 8 * 5 + 8)) == 0
    assert lib.vmasr_dconv1d_wgrad_workspace(8, 8, 1, 5, 1, 2, 8, 120) > 0


def test_dconv1d_launchers_reject_bad_arguments():
    """Refused shapes and null pointers: the invalid-argument code (-1) with a message that states the bounds, nothing launched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused first
    fwd, dgrad, wgrad = lib.vmasr_dconv1d_fwd, lib.vmasr_dconv1d_dgrad, lib.vmasr_dconv1d_wgrad
    big = 1 << 40
    for B, Cin, Cout, groups, L, k, stride, pad in ((2, 8, 8, 1, 20, 5, 2, 2), (2, 8, 8, 2, 20, 5, 1, 2), (2, 8, 8, 1, 20, 5, 1, 5), (2, 8, 8, 1, 20, 9, 1, 2),
                                                    (0, 8, 8, 1, 20, 5, 1, 2), (2, 8, 8, 1, 4, 5, 1, 0), (2, 8, 8, 1, (1 << 28) + 1, 5, 1, 2)):
        geom = (B, Cin, Cout, groups, L, k, stride, pad)
        assert fwd(p, p, p, p, p, p, big, *geom, 1, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error() and b"stride 1" in lib.vmasr_last_error()
        assert dgrad(p, p, p, p, p, big, *geom, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
        assert wgrad(p, p, p, p, p, p, big, *geom, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
    ok = (4, 1024, 1024, 1, 30, 5, 1, 2)          # the forward and the input gradient split K here: they need their workspace
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, p, None, p), (p, p, p, p, None)):          # x, w, y, pre with act
        assert fwd(*args, p, big, *ok, 1, None) == -1
        assert b"null" in lib.vmasr_last_error()
    for args in ((None, p, p, p), (p, p, None, p), (p, p, p, None)):                                     # gy, w, dx
        assert dgrad(*args, p, big, *ok, None) == -1
        assert b"null" in lib.vmasr_last_error()
    assert wgrad(None, p, p, p, p, p, big, *ok, None) == -1 and wgrad(p, None, p, p, p, p, big, *ok, None) == -1
    assert wgrad(p, p, p, None, None, p, big, *ok, None) == -1                                            # nothing wanted
    assert fwd(p, p, p, p, p, None, 0, *ok, 1, None) == -1 and b"workspace" in lib.vmasr_last_error()
    assert fwd(p, p, p, p, p, p, 16, *ok, 1, None) == -1 and b"workspace" in lib.vmasr_last_error()
    assert dgrad(p, p, p, p, p, 16, *ok, None) == -1 and b"workspace" in lib.vmasr_last_error()
    assert wgrad(p, p, p, p, p, p, 16, 8, 8, 8, 1, 120, 5, 1, 2, None) == -1 and b"workspace" in lib.vmasr_last_error()


def test_case_list_reaches_the_tile_edges():
    """What the GPU test's cases are in the list for, computed from the library's constants instead of trusted."""
    from vm_asr_amd import _lib, msd_ops
    lib = _lib.lib()
    P, M, CC, kmax = msd_ops.dconv1d_tiles()
    assert (P, M, CC) == (tc.POS_TILE, tc.M_TILE, tc.K_CHUNK) and P % 16 == 0 and M % 16 == 0
    cases = tc.CASES + [tc.CONV_POST, tc.NO_BIAS[:6]]
    for B, Cin, Cout, L, k, pad in cases:
        assert msd_ops.dconv1d_supported(Cin, Cout, 1, k, 1) and msd_ops.dconv1d_supported_launch(Cin, Cout, 1, k, 1, pad, B, L)
    T = lambda c: c[3] + 2 * c[5] - c[4] + 1
    assert any(T(c) == P + 1 for c in cases) and any(c[3] == P + 1 for c in cases)              # forward / input gradient: one past the tile
    assert any(T(c) == 1 for c in cases) and any(c[3] == 1 for c in cases) and any(T(c) > c[3] for c in cases)
    assert any(c[2] == M + 1 for c in cases) and any(c[1] == M + 1 for c in cases)              # one channel past the M tile of either GEMM
    assert any(c[1] % CC == 1 and c[1] > CC for c in cases) and any(c[2] % CC == 1 and c[2] > CC for c in cases)   # ... past a K chunk
    assert any(c[2] == 1 for c in cases) and any(c[4] == 1 for c in cases) and any(c[4] == kmax for c in cases)
    assert any(c[5] == 0 for c in cases) and any(c[5] == c[4] - 1 for c in cases)
    assert {2 if T(c) <= 32 else 4 if T(c) <= 64 else 8 for c in cases} == {2, 4, 8}             # every position tile
    # K is split, with a short last slab: slabs of `per` chunks, the last one of fewer
    for B, Cin, Cout, L, k, pad in cases:
        S, chunks = msd_ops.dconv1d_fwd_slabs(Cin, Cout, 1, k, 1, pad, B, L), -(-Cin // CC)
        assert 1 <= S <= chunks
        per = -(-chunks // S)
        assert (S - 1) * per < chunks <= S * per                                              # no empty slab
    B, Cin, Cout, L, k, pad = tc.WORKLOAD
    S = msd_ops.dconv1d_fwd_slabs(Cin, Cout, 1, k, 1, pad, B, L)
    assert S > 1 and (Cin // CC) % S == 0 and (Cin // CC) // S > 1                            # the workload: several chunks per slab
    assert any(msd_ops.dconv1d_fwd_slabs(c[1], c[2], 1, c[4], 1, c[5], c[0], c[3]) > 1 and c[1] % CC for c in cases)   # a short last CHUNK
    # the weight gradient: whole-K tiles (no workspace) at the workload, slabs of (b, 32 outputs) units elsewhere, one with a short unit
    ws = lambda c: lib.vmasr_dconv1d_wgrad_workspace(c[1], c[2], 1, c[4], 1, c[5], c[0], c[3])
    assert ws(tc.WORKLOAD) == 0 and any(ws(c) > 0 for c in cases)
    assert any(ws(c) > 0 and T(c) % 32 and T(c) > 32 for c in cases)
    assert any(c[1] > 32 and c[1] % 32 == 1 for c in cases)                                   # a second channel tile of one channel
