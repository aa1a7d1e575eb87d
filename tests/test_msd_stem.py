"""The fused stem of the scale discriminator on the host (no GPU needed): the VMASR_MSD_STEM switch, the C ABI's predicates and
argument checks (csrc/stem1d.hip), and the unchanged torch path of ScaleDiscriminator for CPU tensors."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


def test_msd_stem_switch_is_declared(monkeypatch):
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_MSD_STEM"]
    assert k.default == "hip" and k.values == ("hip", "torch") and k.kind == "choice" and k.reader == "python:msd"
    monkeypatch.delenv("VMASR_MSD_STEM", raising=False)
    assert knobs.get("VMASR_MSD_STEM") == "hip"
    for v in k.values:
        monkeypatch.setenv("VMASR_MSD_STEM", v)
        assert knobs.get("VMASR_MSD_STEM") == v
    monkeypatch.setenv("VMASR_MSD_STEM", "miopen")
    with pytest.raises(ValueError, match="VMASR_MSD_STEM"):
        knobs.get("VMASR_MSD_STEM")


def test_stem1d_predicates():
    from vm_asr_amd import _lib, msd_ops
    lib = _lib.lib()
    q, ql = lib.vmasr_stem1d_supported, lib.vmasr_stem1d_supported_launch
    assert q(128, 15, 1, 7) == 1 and q(1, 1, 1, 0) == 1 and q(16, 32, 1, 31) == 1
    assert q(128, 15, 2, 7) == 0 and q(128, 33, 1, 7) == 0 and q(128, 15, 1, 15) == 0 and q(0, 15, 1, 7) == 0
    assert q(128, 0, 1, 0) == 0 and q(128, 15, 1, -1) == 0
    assert ql(128, 15, 1, 7, 8, 122640) == 1 and ql(1, 1, 1, 0, 1, 1) == 1 and ql(128, 15, 1, 7, 65535, 1 << 28) == 1
    assert ql(128, 15, 1, 7, 0, 100) == 0 and ql(128, 15, 1, 7, 65536, 100) == 0
    assert ql(128, 15, 1, 0, 2, 14) == 0 and ql(128, 15, 1, 0, 2, 15) == 1          # L < k - 2 pad: no output position
    assert ql(128, 4, 1, 0, 2, 3) == 0 and ql(128, 15, 1, 7, 2, 1) == 1
    assert ql(128, 15, 1, 7, 2, (1 << 28) + 1) == 0 and ql(128, 15, 2, 7, 2, 100) == 0
    assert msd_ops.stem1d_supported_launch(128, 15, 1, 7, 8, 122640) and not msd_ops.stem1d_supported_launch(128, 15, 2, 7, 8, 122640)
    assert msd_ops.stem1d_time_tile() >= 64 and msd_ops.stem1d_channel_group() >= 1
    assert lib.vmasr_stem1d_bwd_workspace(128, 15, 1, 7, 8, 122640) > 0
    assert lib.vmasr_stem1d_bwd_workspace(128, 15, 2, 7, 8, 122640) == 0 and lib.vmasr_stem1d_bwd_workspace(128, 15, 1, 7, 0, 100) == 0
    assert lib.vmasr_stem1d_bwd_workspace(128, 33, 1, 7, 8, 100) == 0
    names = [lib.vmasr_prof_name(k) for k in range(_lib.K_COUNT)]
    assert all(n in names for n in (b"stem1d_fwd", b"stem1d_bwd", b"stem1d_bwd_reduce")) and len(set(names)) == _lib.K_COUNT


def test_stem1d_launchers_reject_bad_arguments():
    """Refused shapes and null pointers: the invalid-argument code (-1) before anything is launched."""
    from vm_asr_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(64)          # never dereferenced: every call below is refused first
    fwd, bwd = lib.vmasr_stem1d_fwd, lib.vmasr_stem1d_bwd
    for args in ((None, p, p, p), (p, None, p, p), (p, p, p, None)):                 # x, w, y
        assert fwd(*args, 2, 128, 100, 15, 1, 7, 1, None) == -1
        assert b"null" in lib.vmasr_last_error()
    for geom in ((2, 128, 100, 15, 2, 7), (2, 128, 100, 33, 1, 7), (2, 128, 100, 15, 1, 15), (2, 0, 100, 15, 1, 7), (0, 128, 100, 15, 1, 7),
                 (65536, 128, 100, 15, 1, 7), (2, 128, 14, 15, 1, 0), (2, 128, (1 << 28) + 1, 15, 1, 7)):
        assert fwd(p, p, p, p, *geom, 1, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
        assert bwd(p, p, p, p, p, p, p, p, 1 << 40, *geom, 1, None) == -1
        assert b"unsupported shape" in lib.vmasr_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):                          # gy, x, w
        assert bwd(*args, p, p, p, p, p, 1 << 40, 2, 128, 100, 15, 1, 7, 1, None) == -1
        assert b"null" in lib.vmasr_last_error()
    assert bwd(p, p, p, p, None, None, None, p, 1 << 40, 2, 128, 100, 15, 1, 7, 1, None) == -1      # nothing wanted
    assert bwd(p, p, p, p, None, p, p, p, 16, 2, 128, 100, 15, 1, 7, 1, None) == -1                  # workspace too small
    assert b"workspace" in lib.vmasr_last_error()
    assert bwd(p, p, p, p, None, p, None, None, 0, 2, 128, 100, 15, 1, 7, 1, None) == -1             # dw without a workspace


@pytest.mark.parametrize("mode", ["hip", "torch"])
def test_scale_discriminator_cpu_path_is_unchanged(mode, monkeypatch):
    """CPU tensors: outputs and gradients bit-equal to the plain F.conv1d / F.gelu chain, whatever the switch says."""
    from vm_asr_amd.msd import ScaleDiscriminator, _weight
    monkeypatch.setenv("VMASR_MSD_STEM", mode)
    torch.manual_seed(3)
    D = ScaleDiscriminator(hidden=16).eval()
    x = (0.3 * torch.randn(2, 1, 1201)).requires_grad_()
    score, fmap = D(x)
    (score ** 2).sum().backward()
    got = [score.detach()] + [f.detach() for f in fmap] + [x.grad.clone()] + [p.grad.clone() for p in D.parameters()]
    x.grad = None
    D.zero_grad()
    h, ref_maps = x, []
    for layer in list(D.convs) + [D.conv_post]:
        h = F.conv1d(h, _weight(layer), layer.bias, layer.stride, layer.padding, 1, layer.groups)
        if layer is not D.conv_post:
            h = F.gelu(h)
        ref_maps.append(h)
    ref_score = torch.flatten(h, 1, -1)
    (ref_score ** 2).sum().backward()
    want = [ref_score.detach()] + [f.detach() for f in ref_maps] + [x.grad] + [p.grad for p in D.parameters()]
    assert len(got) == len(want) == 1 + 8 + 1 + len(list(D.parameters()))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
