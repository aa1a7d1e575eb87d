"""The gated Mlp (MODEL.VSSM.GMLP; model/vmamba.py:512-538, :1815) on the CPU: the module against the reference's recorded results
(tests/golden/gmlp.npz, made by tests/golden/make_gmlp_golden.py), the parameter set of a generator built with it, the config
switch, the dispatch predicate and the environment switch of the fused operator (vm_asr_amd/gmlp.py)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmlp.npz")


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def test_gmlp_module_reproduces_the_reference_output_and_gradients():
    """strict=True load of the reference's state_dict (same attribute names and shapes); output and every gradient to 1e-6 of the
    reference's own fp32 run, on plain torch.  The float64 run of the same module is the fixture's adjudicator: the fp32 module
    must be as close to it as the reference's fp32 run is (x 2 + 1e-6)."""
    from vm_asr_amd.vmamba import gMlp
    z = np.load(GOLDEN)
    m = gMlp(16, 64)
    assert [n for n, _ in m.named_children()] == ["fc1", "act", "fc2", "drop"]
    m.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}, strict=True)
    assert tuple(m.fc1.weight.shape) == (128, 16) and tuple(m.fc2.weight.shape) == (16, 64)
    x = torch.from_numpy(z["x"]).requires_grad_()
    y = m(x)
    y.backward(torch.from_numpy(z["gy"]))
    got = {"y": y.detach(), "dx": x.grad, **{f"d::{k}": p.grad for k, p in m.named_parameters()}}
    assert set(got) == {k[5:] for k in z.files if k.startswith("f32::")}
    for k, v in got.items():
        w32, w64 = torch.from_numpy(z[f"f32::{k}"]), torch.from_numpy(z[f"f64::{k}"])
        assert v.shape == w32.shape, k
        assert _rel(v, w32) <= 1e-6, (k, _rel(v, w32))
        assert _rel(v.double(), w64) <= 2 * _rel(w32.double(), w64) + 1e-6, k
    # the halves are not interchangeable: swapping u and z moves the output far beyond the tolerance above
    with torch.no_grad():
        h = m.fc1(x)
        u, zz = h.chunk(2, -1)
        swapped = m.fc2(zz * m.act(u))
    assert _rel(swapped, y.detach()) > 1e-2


def test_channel_first_gmlp_is_the_same_function():
    """channels_first=True: Linear2d on axis 1 and the chunk on axis 1 — the same numbers as the channel-last module on the permuted
    input (module path only: the fused operator never takes it)."""
    from vm_asr_amd import gmlp as G
    from vm_asr_amd.vmamba import gMlp
    torch.manual_seed(0)
    a, b = gMlp(8, 32), gMlp(8, 32, channels_first=True)
    b.load_state_dict({k: v.view(b.state_dict()[k].shape) for k, v in a.state_dict().items()})
    x = torch.randn(2, 3, 5, 8)
    assert torch.allclose(b(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), a(x), atol=1e-6)
    assert b.channel_first and not G.supported(x.permute(0, 3, 1, 2), torch.nn.LayerNorm(8), b)


def _tiny_kw(gmlp):
    return dict(in_chans=1, patch_size=4, depths=[2, 2, 2, 2], dims=8, ssm_d_state=1, ssm_ratio=2.0, ssm_dt_rank="auto",
                ssm_act_layer="silu", ssm_conv=3, ssm_conv_bias=True, ssm_drop_rate=0.0, ssm_init="v0", forward_type="v5",
                mlp_ratio=4.0, mlp_act_layer="gelu", mlp_drop_rate=0.0, gmlp=gmlp, drop_path_rate=0.1, patch_norm=True,
                norm_layer="LN", patchembed_version="v2", downsample_version="v1", upsample_version="v1",
                output_version="v3", concat_skip=True, interact="dual", n_fft=128, hop_length=32, win_length=128,
                spectro_scale="log2", low_freq_replacement=True)


def test_generator_with_gmlp_has_the_reference_parameter_set():
    from vm_asr_amd.model import DualStreamInteractiveMambaUNet
    from vm_asr_amd.vmamba import VSSBlock, gMlp
    z = np.load(GOLDEN)
    m = DualStreamInteractiveMambaUNet(**_tiny_kw(True))
    got = [(k, ",".join(str(int(s)) for s in p.shape)) for k, p in m.named_parameters()]
    want = list(zip([str(k) for k in z["gen_keys"]], [str(s) for s in z["gen_shapes"]]))
    assert got == want
    blocks = [b for b in m.modules() if isinstance(b, VSSBlock)]
    assert blocks and all(isinstance(b.mlp, gMlp) for b in blocks)
    plain = DualStreamInteractiveMambaUNet(**_tiny_kw(False))
    assert not any(isinstance(b.mlp, gMlp) for b in plain.modules() if isinstance(b, VSSBlock))


def test_get_model_honours_the_config_switch():
    import vm_asr_amd
    from vm_asr_amd.config import get_config
    from vm_asr_amd.vmamba import Mlp, VSSBlock, gMlp
    base = ["MODEL.NAME", "DualStreamInteractiveMambaUNet", "MODEL.VSSM.DIMS", 8, "DATA.STFT.N_FFT", 128, "DATA.STFT.WIN_LENGTH", 128]
    for opts, cls in ((["MODEL.VSSM.GMLP", "True"], gMlp), (["MODEL.VSSM.GMLP", True], gMlp), ([], Mlp)):
        cfg = get_config(opts=base + opts)
        assert cfg.MODEL.VSSM.GMLP is (cls is gMlp)
        gen = vm_asr_amd.get_model(cfg)["generator"]
        blocks = [b for b in gen.modules() if isinstance(b, VSSBlock)]
        assert blocks and all(type(b.mlp) is cls for b in blocks)


def test_supported_is_false_off_the_fused_path():
    """CPU tensors, no autocast, d = 1 / 128, another mlp_ratio: the module path.  The width rule is the library's
    (vmasr_gmlp_supported), asked directly where the library is built — it needs no GPU."""
    from vm_asr_amd import _lib, gmlp as G
    from vm_asr_amd.layernorm import LayerNorm
    from vm_asr_amd.vmamba import Mlp, gMlp
    for d, hidden in ((16, 64), (1, 4), (128, 512), (16, 32)):
        x = torch.randn(2, 3, 4, d)
        assert not G.supported(x, LayerNorm(d), gMlp(d, hidden))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert not G.supported(x, LayerNorm(d), gMlp(d, hidden))
    assert not G.supported(torch.randn(2, 3, 4, 16), LayerNorm(16), Mlp(16, 64))
    lib = _lib.lib()
    want = {(8, 32): 1, (16, 64): 1, (32, 128): 1, (64, 256): 1, (1, 4): 0, (128, 512): 0, (16, 32): 0, (16, 128): 0, (24, 96): 0, (0, 0): 0}
    assert {k: lib.vmasr_gmlp_supported(*k) for k in want} == want


def test_entry_points_refuse_a_bad_width_and_no_rows_before_any_launch():
    """No GPU needed: d = 24 and rows = 0 are refused by the host checks, the (host) dummy operands are never touched."""
    import ctypes
    from vm_asr_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_ubyte * 256)(*([0xA5] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL = -1           # include/vmasr_hip.h: contract violated
    for d, rows in ((24, 64), (16, 0), (16, -5), (128, 64)):
        for code in (_lib.torch_dtype_code(torch.float32), _lib.torch_dtype_code(torch.bfloat16)):
            assert lib.vmasr_gmlp_fwd(p, p, p, 1e-5, p, p, p, p, None, 0, p, rows, d, code, None) == EINVAL, (d, rows)
            assert lib.vmasr_last_error().decode().startswith("gmlp_fwd:")
            assert lib.vmasr_gmlp_bwd(p, p, p, p, 1e-5, p, p, p, p, None, 0, p, p, p, p, p, p, p, rows, d, code, None) == EINVAL, (d, rows)
            assert lib.vmasr_last_error().decode().startswith("gmlp_bwd:")
    assert bytes(buf) == b"\xa5" * len(buf)


def test_the_switch_is_declared_and_parsed(monkeypatch):
    from vm_asr_amd import knobs
    k = knobs.KNOBS["VMASR_FUSED_GMLP"]
    assert k.kind == "flag" and k.default is True and k.values == ("0", "1") and k.reader == "python:gmlp"
    monkeypatch.delenv("VMASR_FUSED_GMLP", raising=False)
    assert knobs.get("VMASR_FUSED_GMLP") is True
    for raw, want in (("0", False), ("1", True)):
        monkeypatch.setenv("VMASR_FUSED_GMLP", raw)
        assert knobs.get("VMASR_FUSED_GMLP") is want
    monkeypatch.setenv("VMASR_FUSED_GMLP", "on")
    with pytest.raises(ValueError, match="VMASR_FUSED_GMLP") as e:
        knobs.get("VMASR_FUSED_GMLP")
    assert "on" in str(e.value)
