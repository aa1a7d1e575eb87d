"""Golden fixture of the gated Mlp (MODEL.VSSM.GMLP), made from the REFERENCE on the build machine (tests/golden/_refload.py loads
it from where it lies; nothing of it is copied):

  gmlp.npz  (a) model/vmamba.py:512-538, gMlp(16, 64) (fc1: 16 -> 128, fc2: 64 -> 16, exact GELU, no dropout) on x (2, 5, 7, 16)
                with the incoming gradient gy: the state_dict, and the output, the input gradient and the four parameter
                gradients of the module evaluated in fp32 (`f32::`) and — the same module .double() on the same values — in
                float64 (`f64::`).
            (b) model/model.py, DualStreamInteractiveMambaUNet built with gmlp=True at the tiny size of make_golden.py::gen_model
                (dims 8, n_fft 128): the names (`gen_keys`) and shapes (`gen_shapes`) of its parameters, in order.

    python tests/golden/make_gmlp_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _refload import load_reference  # noqa: E402


def _np(t):
    return t.detach().cpu().numpy().copy()


def _eval(mod, x, gy, dtype):
    mod = copy.deepcopy(mod).to(dtype)
    xi = x.detach().to(dtype).clone().requires_grad_()
    y = mod(xi)
    y.backward(gy.to(dtype))
    out = {"y": _np(y), "dx": _np(xi.grad)}
    out.update({f"d::{k}": _np(p.grad) for k, p in mod.named_parameters()})
    return out


def gen_gmlp(ns):
    out = {}
    torch.manual_seed(51)
    d = 16
    m = ns.vmamba.gMlp(in_features=d, hidden_features=4 * d, act_layer=torch.nn.GELU, drop=0.0, channels_first=False)
    g = torch.Generator().manual_seed(52)
    with torch.no_grad():                      # biases away from their small default range so that the u / z halves differ visibly
        for p in (m.fc1.bias, m.fc2.bias):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(2, 5, 7, d, generator=g)
    gy = torch.randn(2, 5, 7, d, generator=g)
    out.update(x=_np(x), gy=_np(gy))
    out.update({f"sd::{k}": _np(v) for k, v in m.state_dict().items()})
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        out.update({f"{tag}::{k}": v for k, v in _eval(m, x, gy, dt).items()})
    err = np.abs(out["f32::y"] - out["f64::y"]).max() / np.abs(out["f64::y"]).max()
    print(f"  gmlp: |y| max {np.abs(out['f64::y']).max():.4f}, fp32 vs float64 {err:.2e}")

    kw = dict(in_chans=1, patch_size=4, depths=[2, 2, 2, 2], dims=8, ssm_d_state=1, ssm_ratio=2.0,
              ssm_dt_rank="auto", ssm_act_layer="silu", ssm_conv=3, ssm_conv_bias=True,
              ssm_drop_rate=0.0, ssm_init="v0", forward_type="v5", mlp_ratio=4.0,
              mlp_act_layer="gelu", mlp_drop_rate=0.0, gmlp=True, drop_path_rate=0.1,
              patch_norm=True, norm_layer="LN", patchembed_version="v2", downsample_version="v1",
              upsample_version="v1", output_version="v3", concat_skip=True, interact="dual",
              n_fft=128, hop_length=32, win_length=128, spectro_scale="log2",
              low_freq_replacement=True)
    gen = ns.model.DualStreamInteractiveMambaUNet(**kw)
    named = list(gen.named_parameters())
    out["gen_keys"] = np.array([k for k, _ in named])
    out["gen_shapes"] = np.array([",".join(str(int(s)) for s in p.shape) for _, p in named])
    n_gated = sum(1 for k, p in named if k.endswith("mlp.fc1.weight") and p.shape[0] == 2 * 4 * p.shape[1])
    print(f"  generator with gmlp=True: {len(named)} parameters, {n_gated} gated fc1 weights")
    assert n_gated > 0
    np.savez_compressed(os.path.join(HERE, "gmlp.npz"), **out)


if __name__ == "__main__":
    gen_gmlp(load_reference())
