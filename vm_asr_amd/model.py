"""DualStreamInteractiveMambaUNet on the HIP operators (generator of VM-ASR).

Re-statement of the reference generator (model/model.py:119-1003 `MambaUNet`,
:1006-1552 `DualStreamInteractiveMambaUNet`) with IDENTICAL `state_dict` keys and
shapes, so reference checkpoints load with strict=True, and the same constructor
keywords, so `model/__init__.py:get_model`'s call (:12-54) works unchanged.

Data flow (48 kHz: wave (B,1,122640) -> spectrogram 513x512):
    wav2spectro -> split DC bin -> patch-embed (x2 streams) -> 4 encoder stages <-> 4 decoder
    stages (skip concat + 1x1 conv) -> output layer v3 (3 more VSS blocks at 1/4, 1/2, full
    resolution) -> residual on magnitude -> re-attach DC -> spectro2wav.

Reference behaviours that change numerics and are reproduced on purpose:
  * with concat_skip the PHASE stream runs through the MAGNITUDE decoders
    (model/model.py:1186-1187); `layers_decoder_phase` exists in the state_dict but never
    receives a gradient;
  * interaction is sequential: mag += phase, then phase += (new) mag (:1175-1176);
  * low-frequency replacement copies the whole model output (its slice indexes the channel
    axis, :447-451), i.e. it is the identity whenever highcut >= 1 — so the second STFT
    the reference spends there is not recomputed here; the highcut == 0 corner (output
    replaced by the input spectrogram) is kept.

Only the configuration family reachable from configs/*.yaml is built: 4-entry dims,
norm "LN", patch-embed v2, down/upsample v1, output v3, interact dual/m2p/p2m/single.
"""
from collections import OrderedDict
from contextlib import nullcontext as _nullctx
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, knobs
from .stft import spectro2wav, wav2spectro
from .layernorm import LayerNorm
from .linear import Linear as _Linear, linear as _linear
from .vmamba import PatchMerging2D, Permute, VSSBlock, attach_drop_path_pool

__all__ = ["PatchMerging2D", "PatchExpanding", "MambaUNet", "DualStreamInteractiveMambaUNet"]


class PatchExpanding(nn.Module):
    """(B,H,W,C) -> (B,2H,2W,C/2): Linear C->2C, pixel-shuffle, LayerNorm  (model/model.py:92-116)."""

    def __init__(self, dim, dim_scale=2, norm_layer=LayerNorm):
        super().__init__()
        self.dim = dim
        self.expand = _Linear(dim, 2 * dim, bias=False) if dim_scale == 2 else nn.Identity()
        self.norm = norm_layer(dim // dim_scale) if norm_layer is not None else nn.Identity()

    def forward(self, x):
        x = self.expand(x)
        B, H, W, C = x.shape
        c = C // 4
        # "b h w (p1 p2 c) -> b (h p1) (w p2) c"
        x = x.view(B, H, W, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, c)
        return self.norm(x)


class _Im2ColRowsFn(torch.autograd.Function):
    """x (B, C, H, W), any strides -> GEMM rows (B*Ho*Wo, C*kh*kw) in `dtype`, column order (c, i, j) = weight.flatten(1)'s, in one gather
    pass (csrc/im2col.hip: vmasr_im2col2d_rows) instead of F.unfold + a transposing copy (+ a cast); backward: the adjoint gather."""

    @staticmethod
    def forward(ctx, x, k, s, p, dtype):
        import ctypes
        from . import _lib
        B, C, H, W = x.shape
        Ho, Wo = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
        dev = x.device
        cols = torch.empty((B * Ho * Wo, C * k[0] * k[1]), dtype=dtype, device=dev)
        st = (ctypes.c_int64 * 4)(*x.stride())
        _lib.call(_lib.lib().vmasr_im2col2d_rows, x, cols, B, C, H, W, k[0], k[1], s[0], s[1], p[0], p[1], st, _lib.torch_dtype_code(x.dtype),
                  _lib.torch_dtype_code(dtype))
        ctx.geom = (tuple(x.shape), tuple(x.stride()), x.dtype, k, s, p)
        return cols

    @staticmethod
    def backward(ctx, g):
        import ctypes
        from . import _lib
        shape, strides, xdt, k, s, p = ctx.geom
        B, C, H, W = shape
        g = g.contiguous()
        dev = g.device
        dx = torch.empty_strided(shape, strides, dtype=xdt, device=dev)
        st = (ctypes.c_int64 * 4)(*strides)
        _lib.call(_lib.lib().vmasr_col2im2d_rows, g, dx, B, C, H, W, k[0], k[1], s[0], s[1], p[0], p[1], st, _lib.torch_dtype_code(g.dtype),
                  _lib.torch_dtype_code(xdt))
        return dx, None, None, None, None


def _rows_ok(x):
    """dense input (every element of its storage addressed once: empty_strided in the backward is then a plain allocation)"""
    if not knobs.get("VMASR_IM2COL2D") or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    sz = sorted(zip(x.stride(), x.shape))
    exp = 1
    for st, n in sz:
        if n != 1 and st != exp:
            return False
        exp *= n
    return True


class GemmConv2d(nn.Conv2d):
    """nn.Conv2d (same parameters / state_dict keys) evaluated as im2col + GEMM.

    MIOpen has no tuned bf16 solver for the generator's tiny-channel convolutions (1->8 and 8->16
    channels, 3x3 stride 2 on 512x512 / 256x256 planes): it falls back to `naive_conv_*` kernels
    whose weight-gradient alone costs 27-84 ms per call on MI355X (profiles/r01_*).  unfold + a
    hipBLASLt GEMM is the same arithmetic at memory speed."""

    def forward(self, x):
        if not x.is_cuda:
            return super().forward(x)
        B, C, H, W = x.shape
        kh, kw = self.kernel_size
        Ho = (H + 2 * self.padding[0] - kh) // self.stride[0] + 1
        Wo = (W + 2 * self.padding[1] - kw) // self.stride[1] + 1
        if _rows_ok(x) and self.dilation == (1, 1) and self.groups == 1:
            cdt = _lib.autocast_dtype(x)
            if cdt in (torch.float32, torch.bfloat16):
                cols = _Im2ColRowsFn.apply(x, tuple(self.kernel_size), tuple(self.stride), tuple(self.padding), cdt)     # (B*Ho*Wo, C*kh*kw)
                y = _linear(cols, self.weight.flatten(1), self.bias, shadow_of=self.weight)                             # (B*Ho*Wo, Cout)
                return y.view(B, Ho * Wo, -1).transpose(1, 2).reshape(B, -1, Ho, Wo)
        cols = F.unfold(x, self.kernel_size, padding=self.padding, stride=self.stride)  # (B, C*kh*kw, Ho*Wo)
        # pixels as the GEMM's M dimension: (B*Ho*Wo, C*kh*kw) @ (C*kh*kw, Cout).  The batched
        # (Cout x K) @ (K x Ho*Wo) form picks a 32x32 hipBLASLt tile and takes 1.5 ms per call.
        y = _linear(cols.transpose(1, 2), self.weight.flatten(1), self.bias, shadow_of=self.weight)            # (B, Ho*Wo, Cout)
        return y.transpose(1, 2).reshape(B, -1, Ho, Wo)


class PointwiseConvCL(nn.Conv2d):
    """1x1 nn.Conv2d (same parameters / keys) applied to CHANNEL-LAST (B,H,W,C) input as a Linear.
    Replaces the reference's Permute -> Conv2d(1x1) -> Permute sandwiches (model/model.py:917-921,
    862-864) without the two layout copies and without MIOpen's naive 1x1 fallbacks."""

    def forward(self, x):
        return _linear(x, self.weight.flatten(1), self.bias, shadow_of=self.weight)


_ACT = dict(silu=nn.SiLU, gelu=nn.GELU, relu=nn.ReLU, sigmoid=nn.Sigmoid)


def _vss_layer(dim, drop_path, norm_layer, sampler, concat_skip, blk_kw):
    """skip_handler (1x1 conv over the concatenated skip) -> VSSBlocks -> sampler
    (model/model.py:890-958).  Key names: skip_handler.1.*, blocks.N.*, sampler.*"""
    skip = nn.Identity()
    if concat_skip:
        # index 1 keeps the reference's key `skip_handler.1.{weight,bias}`
        skip = nn.Sequential(nn.Identity(), PointwiseConvCL(2 * dim, dim, kernel_size=1), nn.Identity())
    blocks = [VSSBlock(hidden_dim=dim, drop_path=dp, norm_layer=norm_layer, channel_first=False, **blk_kw)
              for dp in drop_path]
    return nn.Sequential(OrderedDict([("skip_handler", skip), ("blocks", nn.Sequential(*blocks)),
                                      ("sampler", sampler)]))


class MambaUNet(nn.Module):
    """Single-stream builder; DualStreamInteractiveMambaUNet deep-copies its parts."""

    def __init__(self, patch_size=4, in_chans=1, depths=[2, 2, 9, 2], dims=[96, 192, 384, 768],
                 ssm_d_state=16, ssm_ratio=2.0, ssm_dt_rank="auto", ssm_act_layer="silu", ssm_conv=3,
                 ssm_conv_bias=True, ssm_drop_rate=0.0, ssm_init="v0", forward_type="v2", mlp_ratio=4.0,
                 mlp_act_layer="gelu", mlp_drop_rate=0.0, gmlp=False, drop_path_rate=0.1, patch_norm=True,
                 norm_layer="LN", patchembed_version="v2", downsample_version="v1", upsample_version="v1",
                 output_version="v2", concat_skip=False, n_fft=512, hop_length=64, win_length=256,
                 spectro_scale="log2", low_freq_replacement=False, **kwargs):
        super().__init__()
        if norm_layer.lower() != "ln":
            raise NotImplementedError("norm_layer: only 'LN' is built (config.py:115; no yaml overrides it)")
        if patchembed_version != "v2" or downsample_version != "v1" or upsample_version != "v1":
            raise NotImplementedError("only patch-embed v2 / downsample v1 / upsample v1 are built (config.py:116-118)")
        if output_version != "v3":
            raise NotImplementedError("only output layer v3 is built (config.py:119; no yaml overrides it)")
        if patch_size != 4:
            raise NotImplementedError("patch_size must be 4 (model/model.py:612)")
        self.channel_first = False
        self.num_layers = len(depths)
        self.depths = list(depths)
        if isinstance(dims, int):
            dims = [int(dims * 2 ** i) for i in range(self.num_layers)]
        if len(dims) != self.num_layers:
            raise NotImplementedError("the 5-entry dims (latent layer) variant is not reachable from any yaml")
        self.dims = list(dims)
        self.num_features = dims[-1]
        self.dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.concat_skip = concat_skip
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.spectro_scale = spectro_scale
        self.low_freq_replacement = low_freq_replacement

        LN = LayerNorm  # nn.LayerNorm subclass on the HIP kernel (same parameters / keys)
        blk_kw = dict(ssm_d_state=ssm_d_state, ssm_ratio=ssm_ratio, ssm_dt_rank=ssm_dt_rank,
                      ssm_act_layer=_ACT[ssm_act_layer.lower()], ssm_conv=ssm_conv, ssm_conv_bias=ssm_conv_bias,
                      ssm_drop_rate=ssm_drop_rate, ssm_init=ssm_init, forward_type=forward_type,
                      mlp_ratio=mlp_ratio, mlp_act_layer=_ACT[mlp_act_layer.lower()], mlp_drop_rate=mlp_drop_rate,
                      gmlp=gmlp)
        d, nl, dep = self.dims, self.num_layers, self.depths

        # patch embed v2 (model/model.py:603-633): 2 stride-2 convs with LN/GELU in between
        e = d[0]
        self.patch_embed = nn.Sequential(
            GemmConv2d(in_chans, e // 2, kernel_size=3, stride=2, padding=1), Permute(0, 2, 3, 1),
            LN(e // 2) if patch_norm else nn.Identity(), Permute(0, 3, 1, 2), nn.GELU(),
            GemmConv2d(e // 2, e, kernel_size=3, stride=2, padding=1), Permute(0, 2, 3, 1),
            LN(e) if patch_norm else nn.Identity())

        self.layers_encoder = nn.ModuleList()
        for i in range(nl):
            down = PatchMerging2D(d[i], d[i + 1], norm_layer=LN) if i < nl - 1 else nn.Identity()
            self.layers_encoder.append(_vss_layer(d[i], self.dpr[sum(dep[:i]):sum(dep[:i + 1])], LN, down, False, blk_kw))
        self.layers_latent = nn.ModuleList()

        # decoders run i_layer = nl .. 1; the first has no blocks (empty drop-path slice) and no sampler
        self.layers_decoder = nn.ModuleList()
        for i in range(nl, 0, -1):
            dim = d[i] if i < nl - 1 else d[nl - 1]
            up = PatchExpanding(d[i], dim_scale=2, norm_layer=LN) if i < nl else nn.Identity()
            self.layers_decoder.append(_vss_layer(dim, self.dpr[sum(dep[:i]):sum(dep[:i + 1])], LN, up,
                                                  concat_skip if i < nl else False, blk_kw))

        # output layer v3 (model/model.py:773-887)
        last = self.dpr[-1:]
        self.output_layer = nn.Sequential(
            _vss_layer(e, last, nn.Identity, PatchExpanding(e, 2, LN), concat_skip, blk_kw),
            _vss_layer(e // 2, last, LN, PatchExpanding(e // 2, 2, LN), False, blk_kw),
            nn.Identity(), PointwiseConvCL(e // 4, in_chans, kernel_size=1), nn.Identity(),  # key `output_layer.3.*`
            _vss_layer(in_chans, last, nn.Identity, nn.Identity(), False, blk_kw),
            Permute(0, 3, 1, 2))
        self.apply(self._init_weights)

    def _init_weights(self, m: nn.Module):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- STFT front-end (model/model.py:424-445) -------------------------------------------
    def _mag_phase(self, x):
        if x.shape[-1] % self.hop_length:
            x = F.pad(x, (0, self.hop_length - x.shape[-1] % self.hop_length))
        return wav2spectro(x, self.n_fft, self.hop_length, self.win_length, self.spectro_scale)

    def _i_mag_phase(self, mag, phase):
        return spectro2wav(mag, phase, self.n_fft, self.hop_length, self.win_length, self.spectro_scale)

    def __str__(self):
        n = sum(p.numel() for p in self.parameters() if p.requires_grad)
        return super().__str__() + f"\nTrainable parameters: {n}"


_PHASE_STREAMS = {}


class _OnMain:
    """(dev aid) a phase-chain segment run on the main stream after all: both streams meet before and after it."""
    def __init__(self, ln):
        self.ln = ln

    def __enter__(self):
        self.ln.main.wait_stream(self.ln.side)

    def __exit__(self, *a):
        self.ln.side.wait_stream(self.ln.main)
        return False


class DualStreamInteractiveMambaUNet(MambaUNet):
    def __init__(self, *args, interact="dual", **kwargs):
        super().__init__(*args, **kwargs)
        if interact not in ("dual", "m2p", "p2m", "single"):
            raise ValueError(f"interact='{interact}'")
        self.interact = interact
        self.patch_embed_mag = deepcopy(self.patch_embed)
        self.layers_encoder_mag = deepcopy(self.layers_encoder)
        self.layers_latent_mag = None
        self.layers_decoder_mag = deepcopy(self.layers_decoder)
        self.output_layer_mag = deepcopy(self.output_layer)
        if interact != "single":
            self.patch_embed_phase = deepcopy(self.patch_embed)
            self.layers_encoder_phase = deepcopy(self.layers_encoder)
            self.layers_latent_phase = None
            self.layers_decoder_phase = deepcopy(self.layers_decoder)
            self.output_layer_phase = deepcopy(self.output_layer)
        del self.patch_embed, self.layers_encoder, self.layers_latent, self.layers_decoder, self.output_layer
        self.apply(self._init_weights)  # the reference re-draws every Linear after the copy
        self._dp_pool = attach_drop_path_pool(self)   # one stochastic-depth draw per forward for all blocks

    def _interact(self, mag, phase):
        if self.interact in ("dual", "p2m"):
            mag = mag + phase
        if self.interact in ("dual", "m2p"):
            phase = phase + mag
        return mag, phase

    # ---- the phase branch on a HIP stream of its own (VMASR_GEN_STREAMS, default "auto": see _lanes) -----------------------------------
    # Between two interaction points the magnitude and the phase branch are independent (different weights in the patch embeddings, the
    # encoders and the output layers; the shared decoders run both stacked).  The generator is ~1 400 launches of 5-20 us, so one branch
    # alone leaves most of the chip idle.  Here the phase branch lives on ONE second stream for the whole forward — two long chains with
    # cross edges at the interaction points (event waits), not a fork / join per stage: in a captured step the runtime gives every fork a
    # stream from its pool, and a per-stage fork lands on the discriminator's branch every so often (measured: generator backward 12.6 ->
    # 17.6 ms beside the D-loss backward).  autograd runs every backward node on its forward's stream, so the backward has the same shape.
    class _Lanes:
        def __init__(self, dev, side):
            self.on = side is not None
            self.main = torch.cuda.current_stream(dev) if self.on else None
            self.side = side
            if self.on:
                side.wait_stream(self.main)

        def phase(self, tag=None):       # context: the phase chain's stream
            if not self.on:
                return _nullctx()
            only = knobs.get("VMASR_GEN_LANES")       # dev aid: which segments leave the main stream (pe,e0..e3,d0..d3,out,ia)
            if only is not None and tag is not None and tag not in only:
                return _OnMain(self)
            return torch.cuda.stream(self.side)

        def to_side(self, *ts):          # tensors produced on main are about to be read on the side stream
            if self.on:
                self.side.wait_stream(self.main)
                for t in ts:     # (also while capturing: the allocator then keeps the block out of reuse until the capture ends)
                    t.record_stream(self.side)

        def to_main(self, *ts):          # tensors produced on the side stream are about to be read on main
            if self.on:
                self.main.wait_stream(self.side)
                for t in ts:
                    t.record_stream(self.main)

    def _lanes(self, x):
        side = None
        mode = knobs.get("VMASR_GEN_STREAMS")
        # In captured steps only (the dependencies are then edges of the graph; "2eager" forces the eager path, a debugging aid), and
        # only with data-parallel library GEMMs (vm_asr_amd/hip_env.py: two concurrent stream-K GEMMs can stop the device).
        # "auto": where the trainer says so (self.phase_lane: generator-only steps, +14 ... +24 % clips/s at batch 35 ... 4) — beside
        # the discriminator's side stream a third stream LOSES (173 -> 147 clips/s at batch 4: profiles/r05_gen_streams_ab.log), so
        # the GAN step keeps the generator on one stream.  "2" / "1" force it on / off.
        want = mode == "2" or (mode == "auto" and getattr(self, "phase_lane", False))
        from . import _lib, hip_env
        # (never in deterministic mode: both branches launch the same ticketed kernels — the tickets are per kernel id, one stream only)
        if (x.is_cuda and self.interact != "single" and hip_env.streamk_dp_in_force() and not _lib.det_mode()
                and (mode == "2eager" or (want and torch.cuda.is_current_stream_capturing()))):
            side = _PHASE_STREAMS.get(x.device)          # (not a module attribute: a Stream cannot be deep-copied with the model)
            if side is None:
                side = _PHASE_STREAMS[x.device] = torch.cuda.Stream(x.device)
        return self._Lanes(x.device, side)

    def _interact_lanes(self, ln, mag, phase):
        """_interact with the magnitude sum on main and the phase sum on the phase chain's stream."""
        if not ln.on:
            return self._interact(mag, phase)
        if self.interact in ("dual", "p2m"):
            ln.to_main(phase)
            mag = mag + phase
        if self.interact in ("dual", "m2p"):
            ln.to_side(mag)
            with ln.phase("ia"):
                phase = phase + mag
        return mag, phase

    def forward(self, x, hf):
        length = x.shape[-1]
        mag_in, phase_in = self._mag_phase(x)          # (B,1,F,M) fp32
        mag_dc, phase_dc = mag_in[..., :1, :], phase_in[..., :1, :]
        mag, phase = mag_in[..., 1:, :], phase_in[..., 1:, :]
        residual_mag = mag
        single = self.interact == "single"

        dev = x.device
        if self.training and self._dp_pool is not None:
            self._dp_pool.refresh(2 * x.shape[0], dev)     # 2B: the shared decoders run both streams stacked
            if x.is_cuda and torch.is_autocast_enabled("cuda"):
                # the table's 16-bit copy, made HERE on the main stream: created lazily by whichever branch asks first it would be
                # written on one stream and read on the other without an edge between them (phase lane, _lanes below)
                self._dp_pool.get(0, 1, 1, torch.get_autocast_dtype("cuda"))
        if not single:
            ln = self._lanes(x)
            ln.to_side(phase)
            with ln.phase("pe"):
                phase = self.patch_embed_phase(phase)
            mag = self.patch_embed_mag(mag)
            skips_m, skips_p = [mag], [phase]
            for i in range(self.num_layers):
                with ln.phase(f"e{i}"):
                    phase = self.layers_encoder_phase[i](phase)
                mag = self.layers_encoder_mag[i](mag)
                if i < self.num_layers - 1:
                    skips_m.append(mag)
                    skips_p.append(phase)
                mag, phase = self._interact_lanes(ln, mag, phase)
            for i in range(self.num_layers):
                dec_m, dec_p = self.layers_decoder_mag[i], self.layers_decoder_phase[i]
                if i != 0:
                    ms, ps = skips_m.pop(), skips_p.pop()
                    if self.concat_skip:
                        # sic: the phase stream also runs through the MAGNITUDE decoder (model/model.py:1187).
                        # Same weights for both streams -> one pass over the stacked batch (identical
                        # arithmetic per sample, half the kernel launches of two separate calls) — on the main stream.
                        ln.to_main(phase, ps)
                        both = dec_m(torch.cat((torch.cat((mag, ms), dim=-1), torch.cat((phase, ps), dim=-1)), dim=0))
                        mag, phase = both[: mag.shape[0]], both[mag.shape[0]:]
                        ln.to_side(phase)
                    else:
                        with ln.phase(f"d{i}"):
                            phase = dec_p(phase + ps)
                        mag = dec_m(mag + ms)
                else:
                    with ln.phase("d0"):
                        phase = dec_p(phase)
                    mag = dec_m(mag)
                mag, phase = self._interact_lanes(ln, mag, phase)
            ms, ps = skips_m.pop(), skips_p.pop()
            with ln.phase("out"):
                phase = self.output_layer_phase(torch.cat((phase, ps), dim=-1) if self.concat_skip else phase + ps)
            mag = self.output_layer_mag(torch.cat((mag, ms), dim=-1) if self.concat_skip else mag + ms)
            ln.to_main(phase)
        else:
            mag = self.patch_embed_mag(mag)
            skips_m = [mag]
            for i in range(self.num_layers):
                mag = self.layers_encoder_mag[i](mag)
                if i < self.num_layers - 1:
                    skips_m.append(mag)
            for i in range(self.num_layers):
                if i != 0:
                    ms = skips_m.pop()
                    mag = self.layers_decoder_mag[i](torch.cat((mag, ms), dim=-1) if self.concat_skip else mag + ms)
                else:
                    mag = self.layers_decoder_mag[i](mag)
            ms = skips_m.pop()
            mag = self.output_layer_mag(torch.cat((mag, ms), dim=-1) if self.concat_skip else mag + ms)

        f32 = (lambda t: t) if mag_in.dtype == torch.float64 else (lambda t: t.float())   # float64: test adjudicator runs
        mag = f32(mag) + residual_mag
        mag = torch.cat([mag_dc, mag], dim=-2)
        if not single:
            phase = torch.cat([phase_dc, f32(phase)], dim=-2)
        else:
            phase = phase_in
        if self.low_freq_replacement:
            # reference: y = spectro(x); y[i, :hf[i], :] = out[i, :hf[i], :] on a (1,F,M) slice ->
            # copies everything unless hf[i] == 0 (model/model.py:447-451,1217-1221)
            keep = (hf.to(mag.device) > 0).view(-1, 1, 1, 1)
            mag = torch.where(keep, mag, mag_in)
            if not single:
                phase = torch.where(keep, phase, phase_in)
        wav = self._i_mag_phase(mag, phase)
        return wav[..., :length]
