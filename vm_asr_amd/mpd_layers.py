"""The stacked layers of the batched period-discriminator pass (discriminator.MultiPeriodDiscriminator._forward_batched): one autograd
function per implementation of a layer (discriminator._layer_path picks), their helpers and the two backward-phase flags."""
import torch
import torch.nn.functional as F

from . import _lib, knobs, mpd_ops as bind
from .linear import _mm_acc
from .mpd_ops import geom_of as _geom, split_bf16


# ---- all period discriminators, layer by layer (stacked GEMM operands) ---------------------------
# The five period discriminators have the same layer shapes and nearly the same number of GEMM rows
# (B*p*T'_p ~ B*T/3^l for every p), but run one after the other each of their GEMMs fills a fraction of the
# 256 CUs (M ~ 4.7 k rows x N = 1024: 76 tiles of 256x256).  Stacked into one batched GEMM per layer they
# fill the chip, and GELU / bias / weight casts run once per layer instead of once per discriminator.

def _round_up(v, m):
    return -(-v // m) * m


class _StackedIm2ColFn(torch.autograd.Function):
    """n channel-last inputs (B, P_i, H_i, C) -> one (n, rows, k*C) column tensor, slot i holding the im2col
    of input i in its first B*P_i*H1_i rows and zeros below (vmasr_im2col_kx1 with rows_out).
    geom = ((N_i, H_i), ...) : the n inputs are the slots of ONE stacked tensor xs[0] (n, rows_in, C), slot i holding N_i
    sequences of H_i positions in its first rows (the previous layer's stacked output); the backward then writes the
    stacked gradient directly (no per-slot tensors, no re-stacking)."""

    @staticmethod
    def forward(ctx, k, stride, pad, rows, geom, *xs):
        if geom is not None:
            src = xs[0].contiguous()
            ctx.geom = (k, stride, pad, None, tuple(geom), tuple(src.shape))
        else:
            src, geom = [x.contiguous() for x in xs], _geom(xs)
            ctx.geom = (k, stride, pad, [tuple(x.shape) for x in xs], None, None)
        return bind.im2col_kx1(src, geom, src[0].shape[-1], k, stride, pad, rows)

    @staticmethod
    def backward(ctx, g):
        k, stride, pad, shapes, geom, sshape = ctx.geom
        g = g.contiguous()
        if geom is not None:
            return (None, None, None, None, None, bind.col2im_kx1_stacked(g, geom, sshape, k, stride, pad))
        return (None, None, None, None, None, *bind.col2im_kx1_multi(g, shapes, k, stride, pad))


class _PhaseFlag:
    """`with flag():` sets the class' `on` for the block and restores the value it found (nesting, exceptions)."""
    on = False

    def __enter__(self):
        self._saved, type(self).on = type(self).on, True

    def __exit__(self, *exc):
        type(self).on = self._saved


class skip_weight_grads(_PhaseFlag):
    """Backward-phase switch of the trainer's shared fake pass: while the GENERATOR loss is back-propagated through the discriminator's
    graph only the column / input gradients are wanted; the weight gradients belong to the discriminator loss' own backward through it."""


class scores_only(_PhaseFlag):
    """with scores_only(): the loss being back-propagated reads the discriminator's SCORES only (the discriminator loss of
    model/loss.py:190-213), no feature map: a map's only consumer is then the layer above it, which may finish the layer's activation
    backward — GELU', bf16 split, bias-gradient column sums — in its input-gradient epilogue (_Link.plan)."""


class _BatchedLinearFn(torch.autograd.Function):
    """y[i] = cols[i] @ W[i]^T + b[i] for the n stacked discriminators (one batched GEMM); backward: one batched
    GEMM for the column gradient, the weight gradient split over the rows into a larger batch (fp32 sum)."""

    @staticmethod
    def forward(ctx, cols, weight, bias, cdt, act=False):
        """act: GELU on the output; for fp32 operands on the GPU the bias + GELU epilogue and, in the backward, GELU' + the
        bias gradient are single passes (csrc/split.hip) instead of add_, gelu, gelu_backward and a column sum."""
        wc = weight.detach().to(cdt)                                   # (n, N, K): the operand of dcols = gy @ W
        # The forward operand is a CONTIGUOUS (n, K, N) copy: batched bf16 GEMMs with a transposed-view B operand
        # fault the GPU on ROCm 7.2 / hipBLASLt for e.g. (5, 36608, 640) x (5, 640, 512)^T (tools/bmm_probe.py);
        # contiguous-B ("NN") and transposed-A ("TN", the weight gradient) forms are fine at every MPD shape.
        y = torch.bmm(cols, wc.transpose(1, 2).contiguous())
        n, M, N = y.shape
        fused = act and y.is_cuda and y.dtype == torch.float32 and N % 4 == 0 and N <= 1024
        pre = None
        if fused:
            pre = y
            y = bind.bias_gelu_fwd(pre, bias.detach().float().contiguous())
        else:
            y.add_(bias.detach().to(cdt).unsqueeze(1))
            if act:
                pre = y
                y = F.gelu(pre)
        ctx.save_for_backward(cols, wc, *([pre] if pre is not None else []))
        ctx.meta = (weight.dtype, bias.dtype, act, fused)
        return y

    @staticmethod
    def backward(ctx, gy):
        cols, wc, *rest = ctx.saved_tensors
        wdt, bdt, act, fused = ctx.meta
        gy = gy.contiguous()
        n, M, N = gy.shape
        K = cols.shape[2]
        skip_w = skip_weight_grads.on
        db = None
        if fused:
            want_db = ctx.needs_input_grad[2] and not skip_w
            gy, db32 = bind.gelu_bwd(rest[0], gy, want_db=want_db)
            db = db32.to(bdt) if want_db else None
        elif act:
            gy = torch.ops.aten.gelu_backward(gy, rest[0])
        dcols = torch.bmm(gy, wc) if ctx.needs_input_grad[0] else None
        dw = None
        if skip_w:
            return dcols, None, None, None, None
        if ctx.needs_input_grad[1]:
            acc = torch.float32 if gy.dtype in (torch.float16, torch.bfloat16) else gy.dtype
            tiles = n * -(-N // 64) * -(-K // 64)
            want = min(M // 2048, max(1, 512 // tiles))
            S = max(d for d in range(1, max(1, want) + 1) if (M // 256) % d == 0) if M % 256 == 0 else 1
            if S > 1:   # (n, S, M/S, .) -> batch n*S: the row split is a free view because S divides M
                part = _mm_acc(gy.view(n * S, M // S, N).transpose(1, 2), cols.view(n * S, M // S, K), acc)
                dw = part.view(n, S, N, K).sum(1)
            else:
                dw = _mm_acc(gy.transpose(1, 2), cols, acc)
            dw = dw.to(wdt)
        if ctx.needs_input_grad[2] and not fused:
            db = gy.sum(1, dtype=torch.float32 if gy.dtype in (torch.float16, torch.bfloat16) else None).to(bdt)
        return dcols, dw, db, None, None


def _bmm3(ah, al, bh, bl):
    """(ah + al) @ (bh + bl) without the lo*lo term: three bf16 MFMA GEMMs, fp32 output and accumulation."""
    f32 = torch.float32
    y = torch.bmm(ah, bh, out_dtype=f32)
    y += torch.bmm(al, bh, out_dtype=f32)
    y += torch.bmm(ah, bl, out_dtype=f32)
    return y


def _split_k(n, N, K, M):
    """Split factor S of the weight-gradient GEMM's contraction (M rows): hipBLASLt runs these as 256x256 macro
    tiles, so a (N, K) output with few tiles leaves most of the 256 CUs idle unless the contraction is spread over
    S batches.  Measured on MI355X (tools/bench_gemm.py, profiles/r02_gemm_layouts.log): 512x640 (30 tiles for five
    slots) 203 us at S=1, 80 us at S=8; 1024x5120 (400 tiles = 1.56 waves of CUs) 491 us at S=1, 362 us at S=3;
    1024x2560 is flat (190 / 182 us)."""
    if M % 256:
        return 1
    tiles = n * -(-N // 256) * -(-K // 256)
    blocks = M // 256
    if tiles <= 64:
        want = 8
    elif 256 < tiles < 512:
        want = 3
    else:
        return 1
    return max(d for d in range(1, want + 1) if blocks % d == 0)


def _dw3(gh, gl, ch, cl, wdt):
    """dW = (gh + gl)^T (ch + cl) without lo*lo over the stacked rows: the three products of all S contraction
    slabs land in ONE (3, n*S, N, K) buffer that a single reduction sums (instead of two read-modify-write passes
    plus a slab sum)."""
    n, M, N = gh.shape
    K = ch.shape[2]
    S = _split_k(n, N, K, M)
    v = (lambda t: t.view(n * S, M // S, t.shape[2])) if S > 1 else (lambda t: t)
    ght, glt = v(gh).transpose(1, 2), v(gl).transpose(1, 2)
    parts = torch.empty((3, n * S, N, K), dtype=torch.float32, device=gh.device)
    torch.bmm(ght, v(ch), out_dtype=torch.float32, out=parts[0])
    torch.bmm(glt, v(ch), out_dtype=torch.float32, out=parts[1])
    torch.bmm(ght, v(cl), out_dtype=torch.float32, out=parts[2])
    if (N * K) % 4 == 0 and n <= 65535:
        return bind.sum_parts(parts, 3, n, S, (N, K)).to(wdt)
    return parts.view(3, n, S, N, K).sum((0, 2)).to(wdt)


def _split_mode(K, N, cdt):
    """Which GEMMs of the fp32 discriminator run as error-compensated bf16 triples: the compute-bound ones
    (K*N >= 2^18: the 128->512, 512->1024 and 1024->1024 convolutions, 98 % of the FLOPs); the two small-K layers
    are memory-bound and stay plain fp32 GEMMs.  VMASR_MPD_GEMM=fp32 switches the triples off."""
    return (cdt == torch.float32 and K * N >= knobs.get("VMASR_MPD_SPLIT_MIN")
            and knobs.get("VMASR_MPD_GEMM") == "bf16x3")


class _BatchedLinearSplitFn(torch.autograd.Function):
    """_BatchedLinearFn for fp32 operands on the bf16 matrix cores: every GEMM (y, dcols, dW) is the
    error-compensated triple hi*hi + lo*hi + hi*lo of bf16 splits (csrc/split.hip), accumulated in fp32 —
    the fp32 result to ~1e-6 relative at 16/3 of the fp32 MFMA rate."""

    @staticmethod
    def forward(ctx, cols, weight, bias):
        ch, cl = split_bf16(cols)                                        # (n, M, K)
        w = weight.detach().float()
        wh, wl = split_bf16(w)                                           # (n, N, K): operand of dcols = gy @ W
        wth, wtl = split_bf16(w.transpose(1, 2).contiguous())            # (n, K, N): contiguous B operand (see _BatchedLinearFn)
        y = _bmm3(ch, cl, wth, wtl).add_(bias.detach().float().unsqueeze(1))
        ctx.save_for_backward(ch, cl, wh, wl)
        ctx.meta = (weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        ch, cl, wh, wl = ctx.saved_tensors
        wdt, bdt = ctx.meta
        gy = gy.float().contiguous()
        n, M, N = gy.shape
        K = ch.shape[2]
        gh, gl = split_bf16(gy)
        dcols = _bmm3(gh, gl, wh, wl) if ctx.needs_input_grad[0] else None
        if skip_weight_grads.on:
            return dcols, None, None
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = _dw3(gh, gl, ch, cl, wdt)
        if ctx.needs_input_grad[2]:
            db = gy.sum(1).to(bdt)
        return dcols, dw, db


class _StackedConvSplitFn(torch.autograd.Function):
    """_StackedIm2ColFn + _BatchedLinearSplitFn as one function for fp32 inputs: the im2col kernel writes the bf16
    hi / lo operands directly (no fp32 column tensor, no separate split pass); the column gradient is ONE GEMM over
    the concatenated contraction [gh | gl | gh] @ [wh; wh; wl] (the three products accumulate inside the GEMM
    instead of two read-modify-write passes over the (rows, k*C) gradient), then col2im per slot."""

    @staticmethod
    def forward(ctx, k, stride, pad, rows, act, geom, weight, bias, *xs):
        """act: apply GELU to the output inside (epilogue kernel; the backward then fuses GELU', the bias gradient
        and the bf16 split of the incoming gradient into one pass, csrc/split.hip).
        geom = ((N_i, H_i), ...): the inputs are the slots of ONE stacked fp32 tensor xs[0] (n, rows_in, C) — the previous
        layer's stacked output — and the backward returns its stacked gradient (see _StackedIm2ColFn)."""
        sgeom = tuple(geom) if geom is not None else None
        if geom is not None:
            src = xs[0].float().contiguous()
        else:
            src, geom = [x.float().contiguous() for x in xs], _geom(xs)
        C, dev = xs[0].shape[-1], xs[0].device
        n, K = len(geom), k * C
        w = weight.detach().float().contiguous()
        N = w.shape[1]
        fused = act and N % 4 == 0 and N <= 1024
        kcat = fused and knobs.get("VMASR_MPD_KCAT")
        if kcat:
            # (opt-in, VMASR_MPD_KCAT=1 — measured SLOWER in round 3: 38.8 vs 38.0 ms per step.  The epilogue gains 0.36 ms
            #  (one partial product to read instead of three), but im2col writes a third operand block (+0.25 ms) and
            #  hipBLASLt's kernels for K' = 3K with M = 4.7k .. 36k are slower than three K-sized products (+0.9 ms).)
            # ONE operand [hi | lo | hi] (n, rows, 3K): the forward triple as a single GEMM over the concatenated contraction;
            # hi / lo stay addressable as column blocks (ld = 3K) for the weight-gradient GEMMs
            acat = bind.im2col_kx1_split(src, geom, C, k, stride, pad, rows, cat3=True)
            ch, cl = acat[:, :, :K], acat[:, :, K:2 * K]
        else:
            ch, cl = bind.im2col_kx1_split(src, geom, C, k, stride, pad, rows)
        # weights: one pass to the (n, K, 3N) bf16 operand [hi^T | hi^T | lo^T] (csrc/split.hip): column blocks 0 and 2 are
        # the forward B operands; all of it, transposed, is the [wh; wh; wl] operand of the column-gradient GEMM
        # (kept as the transpose of a contiguous tensor: hipBLASLt's kernels for that layout are ~9 % faster here)
        wcat = bind.weight_prep_split(w)
        wth, wtl = wcat[:, :, :N], wcat[:, :, 2 * N:]
        b32 = bias.detach().float().contiguous()
        pre = None
        if kcat:
            f32 = torch.float32
            wk = torch.cat((wth, wth, wtl), dim=1)                       # (n, 3K, N) = [w_hi^T; w_hi^T; w_lo^T]
            pre = torch.bmm(acat, wk, out_dtype=f32)
            y = bind.bias_gelu_fwd(pre, b32)
        elif fused:
            # the three products side by side; the epilogue sums them, adds the bias (-> pre, in place in part 0) and applies GELU
            f32 = torch.float32
            parts = torch.empty((3, n, rows, N), dtype=f32, device=dev)
            torch.bmm(ch, wth, out_dtype=f32, out=parts[0])
            torch.bmm(cl, wth, out_dtype=f32, out=parts[1])
            torch.bmm(ch, wtl, out_dtype=f32, out=parts[2])
            pre = parts[0]
            y = bind.bias_gelu_fwd(parts, b32, 3)
        else:
            y = _bmm3(ch, cl, wth, wtl)
            y.add_(b32.unsqueeze(1))
            if act:
                pre = y
                y = F.gelu(pre)
        ctx.save_for_backward(ch, cl, wcat, *([pre] if pre is not None else []))
        ctx.geom = (k, stride, pad, [tuple(x.shape) for x in xs], weight.dtype, bias.dtype, [x.dtype for x in xs], act, fused, sgeom)
        return y

    @staticmethod
    def backward(ctx, gy):
        ch, cl, wcat, *rest = ctx.saved_tensors
        k, stride, pad, shapes, wdt, bdt, xdts, act, fused, sgeom = ctx.geom
        gy = gy.float().contiguous()
        n, M, N = gy.shape
        K = ch.shape[2]
        want_db = ctx.needs_input_grad[7] and not skip_weight_grads.on
        want_dx = any(ctx.needs_input_grad[8:])
        db32 = gcat = None
        if N % 4 == 0 and N <= 1024:
            # one pass: (GELU' *) gradient -> bf16 split (+ bias gradient); the fp32 gradient is never written
            # (with an input gradient wanted as [gh | gl | gh]: the weight-gradient GEMMs read gh, gl as column blocks of it, lda = 3N)
            db32, = _lib.zeros_f32(gy.device, (n, N) if want_db else None)
            gh, gl, gcat = bind.gelu_bwd_split(rest[0] if act else None, gy, db32, cat=want_dx)
        else:
            if act:
                gy = torch.ops.aten.gelu_backward(gy, rest[0])
            gh, gl = split_bf16(gy)
            db32 = gy.sum(1) if want_db else None
        dxs = [None] * len(shapes)
        if want_dx:
            if gcat is None:
                gcat = torch.cat((gh, gl, gh), dim=2)
            dcols = torch.bmm(gcat, wcat.transpose(1, 2), out_dtype=torch.float32)
            if sgeom is not None:      # stacked input: its stacked gradient in one launch (zero rows below each slot's data)
                dxs = [bind.col2im_kx1_stacked(dcols, sgeom, shapes[0], k, stride, pad).to(xdts[0])]
            else:
                outs = bind.col2im_kx1_multi(dcols, shapes, k, stride, pad, ctx.needs_input_grad[8:])
                dxs = [o.to(xdts[i]) if o is not None else None for i, o in enumerate(outs)]
        dw = db = None
        if not skip_weight_grads.on:
            if ctx.needs_input_grad[6]:
                dw = _dw3(gh, gl, ch, cl, wdt)
            if ctx.needs_input_grad[7]:
                db = db32.to(bdt)
        return (None, None, None, None, None, None, dw, db, *dxs)


def _dgrad_operand(ops, key, pair, w, k, n, N, C):
    """W (n, Cout, k*C) -> (n, C, k*Cout) fp32 or its bf16 pair, (tap, output channel) order: the input gradient's B operand, kept in `ops`"""
    if key not in ops:
        if bind.weight_transpose_supported(N, C):      # transposed (and split) in one pass through LDS tiles (csrc/split.hip)
            ops[key] = bind.weight_transpose(w, k, pair=pair)
        else:
            wt = w.view(n, N, k, C).permute(0, 3, 2, 1).reshape(n, C, k * N).contiguous()
            ops[key] = split_bf16(wt) if pair else wt
    return ops[key]


class _StackedConvMfmaFn(torch.autograd.Function):
    """One stacked (k,1) convolution + bias + GELU of the n period discriminators as ONE implicit bf16x3 MFMA GEMM launch
    each way (csrc/convgemm.hip, vm_asr_amd/convgemm.py) — no im2col operand, no partial products, no col2im.
    x (n, rows_in, C) fp32 stacked input (slot i: N_i sequences of H_i positions), pair = its bf16 (hi, lo) split if the
    producing layer already wrote it; W (n, Cout, k*C) fp32 in (tap, channel) order; returns y = GELU(conv + bias) stacked
    (n, rows, Cout) and leaves the pair of y in `link.pair` for the next layer.  wcache: dict shared by the passes of a step
    while the weights are frozen (the split / transposed-split operands of W are built once per step)."""

    @staticmethod
    def forward(ctx, k, stride, pad, rows, geom, wcache, weight, bias, x, xh, xl, link, below=None, wpair=None):
        """wpair: the bf16 pair of `weight` where its producer wrote it (_SNStackFn), else it is split here.  link / below: the _Link shared
        with the layer above / below (link: always a _Link, filled here; below None: no fusion across that boundary).  The backward of
        the layer ABOVE may finish this layer's activation backward in its input-gradient epilogue (csrc/convgemm.hip EPI 2) and put()
        the result into `link`; this layer's backward then starts from link.take() (see _fuse_below)."""
        from . import convgemm as cg
        x_req = x.requires_grad
        x = x.float().contiguous()
        w = weight.detach().float().contiguous()
        f32 = x.shape[2] < 128 and _l1_mode() == "f32"       # the 32 -> 128 layer: exact-f32 products, forward and input gradient
        ops = wcache.get("ops") if wcache is not None else None
        if ops is None:
            ops = {} if f32 else {"w": wpair if wpair is not None else split_bf16(w)}
            if wcache is not None:
                wcache["ops"] = ops
        if f32:
            pre, y, yh, yl = cg.conv_fwd_f32(x, w, bias.detach().float().contiguous(), geom, k, stride, pad, rows, act=True)
            xh = xl = x                                       # (the bf16 pair of x is made in the backward, where the weight gradient wants it)
        else:
            if xh is None:
                xh, xl = split_bf16(x)
            wh, wl = ops["w"]
            pre, y, yh, yl = cg.conv_fwd(xh, xl, wh, wl, bias.detach().float().contiguous(), geom, k, stride, pad, rows, act=True)
        ctx.save_for_backward(xh, xl, pre, w)
        ctx.f32 = f32
        ctx.meta = (k, stride, pad, tuple(geom), ops, weight.dtype, bias.dtype, x.shape)
        ctx.link, ctx.below = link, below
        link.fill(pre, x.shape[2], x_req, weight.requires_grad, bias.requires_grad, pair=(yh, yl))
        return y

    @staticmethod
    def _fuse_below(ctx, gh, gl, wth, wtl, geom, k, stride, pad, rows_in, skip_w):
        """Input gradient of this layer + the activation backward of the layer below in one launch, if that layer can start from it:
        -> True (result put() into the link below; the caller returns a poisoned placeholder as dx) or False (nothing done).  The bias
        gradient's column sums and the feature-matching term of the map between the two layers are part of the epilogue."""
        from . import convgemm as cg
        plan = ctx.below.plan(skip_w, scores_only.on) if ctx.below is not None else None
        if plan is None:
            return False
        db32 = _lib.zeros_f32(gh.device, (gh.shape[0], wth.shape[1]))[0] if plan.want_db else None
        g32, pair = cg.conv_dgrad_gelu(gh, gl, wth, wtl, geom, k, stride, pad, rows_in, ctx.below.pre, want_f32=plan.want_f32,
                                       want_pair=plan.want_pair, db=db32, **(plan.loss or {}))
        ctx.below.put(g32, pair, db32)
        return True

    @staticmethod
    def backward(ctx, gy):
        from . import convgemm as cg
        xh, xl, pre, w = ctx.saved_tensors
        k, stride, pad, geom, ops, wdt, bdt, xshape = ctx.meta
        n, M, N = gy.shape
        C = xshape[2]
        skip_w = skip_weight_grads.on
        want_db = ctx.needs_input_grad[7] and not skip_w
        # The input gradient of the 32 -> 128 layer stays FP32 arithmetic: it is the last GEMM in front of d(loss)/d(wave), a sum with heavy
        # cancellation, where the pair's 16-17 bits per product showed (2.5e-3 of the gradient's scale from float64 against 4e-4 for fp32 —
        # tests/test_mpd.py holds 5e-4).  Default (ctx.f32): the exact-f32 MFMA implicit GEMM; VMASR_MPD_CONV_L1=1: fp32 library GEMM + col2im.
        # The weight gradient takes the bf16x3 kernel like the other layers
        fp32_dgrad = C < 128 and ctx.needs_input_grad[8]
        need_pair = (not fp32_dgrad and ctx.needs_input_grad[8]) or (ctx.needs_input_grad[6] and not skip_w)
        gh = gl = gx = None
        stash = ctx.link.take()
        if stash is not None:      # the layer above has already applied GELU' (and the feature-matching term): gy is a placeholder
            gx, pair_, db32 = stash
            gh, gl = pair_ if pair_ is not None else (None, None)
            if (want_db and db32 is None) or (need_pair and gh is None) or (fp32_dgrad and gx is None):
                raise RuntimeError("MPD: the fused activation backward left less than this layer's backward needs")
        if stash is None:
            gy = gy.float().contiguous()
            db32, = _lib.zeros_f32(gy.device, (n, N) if want_db else None)
            if need_pair:
                gh, gl, _ = bind.gelu_bwd_split(pre, gy, db32)
            if fp32_dgrad:
                gx, _ = bind.gelu_bwd(pre, gy, None if need_pair else db32)
        dx = dw = db = None
        if fp32_dgrad and ctx.f32:
            dx = cg.conv_dgrad_f32(gx, _dgrad_operand(ops, "wt32", False, w, k, n, N, C), geom, k, stride, pad, xshape[1])      # exact-f32 implicit GEMM: no column operand, no col2im
        elif fp32_dgrad:
            dx = bind.col2im_kx1_stacked(torch.bmm(gx, w), geom, xshape, k, stride, pad)      # dcols (n, M, k*C) fp32
        elif ctx.needs_input_grad[8]:
            wth, wtl = _dgrad_operand(ops, "wt", True, w, k, n, N, C)
            if _StackedConvMfmaFn._fuse_below(ctx, gh, gl, wth, wtl, geom, k, stride, pad, xshape[1], skip_w):
                dx = _poison(gy.device).expand(xshape)      # nobody may read it: the layer below starts from ctx.below.take()
            else:
                dx = cg.conv_dgrad(gh, gl, wth, wtl, geom, k, stride, pad, xshape[1])
        if not skip_w:
            if ctx.needs_input_grad[6]:
                if ctx.f32:
                    xh, xl = split_bf16(xh)                                # (saved as the fp32 input)
                dw = cg.conv_wgrad(gh, gl, xh, xl, geom, k, stride, pad).to(wdt)
            if want_db:
                db = db32.to(bdt)
        return (None, None, None, None, None, None, dw, db, dx, None, None, None, None, None)


_POISON = {}


def _poison(device):
    """A NaN scalar: expanded to the shape of a gradient that must not be read (its content travelled another way)."""
    t = _POISON.get(device)
    if t is None:
        t = _POISON[device] = torch.full((), float("nan"), dtype=torch.float32, device=device)
    return t


def _l1_mode():
    """how the 32 -> 128 layer runs: "f32" (default) exact-f32 MFMA implicit GEMM, "1" bf16x3 pairs (forward below the accuracy gate), "0" library GEMMs"""
    return knobs.get("VMASR_MPD_CONV_L1")


class _StackedConvFirstFn(torch.autograd.Function):
    """The first convolution (1 -> 32 channels, kernel (5,1), stride (3,1), padding 2) + GELU of all n period discriminators
    in one launch on the folded signals xs[i] (B, p, H, 1) — csrc/convfirst.hip — instead of a 5-column im2col operand, a
    K = 5 GEMM and an epilogue pass.  W (n, 32, 5), bias (n, 32).  Returns the stacked activations (n, rows, 32)."""

    @staticmethod
    def forward(ctx, rows, W, bias, *xs):
        xcs = [x.float().contiguous() for x in xs]
        w32, b32 = W.detach().float().contiguous(), bias.detach().float().contiguous()
        pre, act = bind.conv_first_fwd(xcs, _geom(xcs), w32, b32, rows)
        ctx.save_for_backward(pre, w32, *xcs)
        ctx.meta = (W.dtype, bias.dtype, [x.dtype for x in xs], [tuple(x.shape) for x in xs])
        return act

    @staticmethod
    def backward(ctx, gy):
        pre, w32, *xcs = ctx.saved_tensors
        wdt, bdt, xdts, shapes = ctx.meta
        gy = gy.float().contiguous()
        skip_w = skip_weight_grads.on
        want_dw, want_db = ctx.needs_input_grad[1] and not skip_w, ctx.needs_input_grad[2] and not skip_w
        want_dx = any(ctx.needs_input_grad[3:])
        dxs = [None] * len(xcs)
        dcols, dw, db = bind.conv_first_bwd(xcs, _geom(shapes), w32, pre, gy, want_dx, want_dw, want_db)
        if want_dx:
            outs = bind.col2im_kx1_multi(dcols, shapes, 5, 3, 2, ctx.needs_input_grad[3:])
            dxs = [o.to(xdts[i]) if o is not None else None for i, o in enumerate(outs)]
        return (None, dw.to(wdt) if want_dw else None, db.to(bdt) if want_db else None, *dxs)


class _StackedConvPostFn(torch.autograd.Function):
    """conv_post (C -> 1 channels, kernel (3,1), stride 1, padding 1) of all n period discriminators directly on the previous
    layer's stacked output x (n, rows, C) — csrc/convpost.hip: one streaming pass forward, one backward, instead of a
    (rows, 3C) im2col operand feeding a GEMV.  W (n, 1, 3C) in (tap, channel) order, bias (n, 1); Ms[i] valid rows =
    whole sequences of Hs[i] positions.  Returns (n, rows, 1).
    below: the _Link of the _StackedConvMfmaFn layer that produced x (None: no fusion across this boundary): the backward may finish
    that layer's activation backward in its own launch (vmasr_conv_post_bwd_gelu) and put() the result into it (see _fuse_below)."""

    @staticmethod
    def forward(ctx, Ms, Hs, W, bias, x, below=None):
        xc, w32, b32 = x.contiguous(), W.detach().float().contiguous(), bias.detach().float().contiguous()
        y = bind.conv_post_fwd(xc, w32, b32, Ms, Hs)
        ctx.save_for_backward(xc, w32)
        ctx.meta = (tuple(Ms), tuple(Hs), W.dtype, bias.dtype, tuple(bias.shape))
        ctx.below = below
        return y

    @staticmethod
    def _fuse_below(ctx, xc, w32, gy, Ms, Hs, want_dw, want_db, skip_w):
        """The input gradient of conv_post + the activation backward of the layer below in one launch, under the conditions of
        _Link.plan, the map being x itself: -> (dw, db) with the result put() into the link below (the caller returns a poisoned
        placeholder as dx), or None (nothing done)."""
        plan = ctx.below.plan(skip_w, scores_only.on, map_shape=xc.shape) if ctx.below is not None else None
        if plan is None:
            return None
        g32, pair, dbcol, dw, db = bind.conv_post_bwd_gelu(xc, w32, gy, ctx.below.pre, Ms, Hs, plan.want_pair, plan.want_f32, want_dw, want_db,
                                                           plan.want_db, **(plan.loss or {}))
        ctx.below.put(g32, pair, dbcol)
        return dw, db

    @staticmethod
    def backward(ctx, gy):
        xc, w32 = ctx.saved_tensors
        Ms, Hs, wdt, bdt, bshape = ctx.meta
        gy = gy.float().contiguous()
        skip_w = skip_weight_grads.on
        want_dx, want_dw, want_db = ctx.needs_input_grad[4], ctx.needs_input_grad[2] and not skip_w, ctx.needs_input_grad[3] and not skip_w
        fused = _StackedConvPostFn._fuse_below(ctx, xc, w32, gy, Ms, Hs, want_dw, want_db, skip_w) if want_dx else None
        if fused is not None:
            (dw, db), dx = fused, _poison(gy.device).expand(xc.shape)      # nobody may read it: the layer below starts from ctx.below.take()
        else:
            dx, dw, db = bind.conv_post_bwd(xc, w32, gy, Ms, Hs, want_dx, want_dw, want_db)
        return (None, None, dw.to(wdt) if want_dw else None, db.view(bshape).to(bdt) if want_db else None, dx, None)


class _UnstackRowsFn(torch.autograd.Function):
    """(n, rows, N) -> n views y[i, :M_i]; the backward assembles the stacked gradient with one copy per slot
    (autograd's own select/slice backward would zero-fill a full-size tensor per slot)."""

    @staticmethod
    def forward(ctx, y, *Ms):
        ctx.shape = tuple(y.shape)
        ctx.Ms = Ms
        return tuple(y[i, :m] for i, m in enumerate(Ms))

    @staticmethod
    def backward(ctx, *gs):
        ref = next(g for g in gs if g is not None)
        if ref.is_cuda and len(gs) <= 8:
            return (bind.stack_rows(gs, ctx.Ms, ctx.shape, ref), *([None] * len(ctx.Ms)))
        full = torch.empty(ctx.shape, dtype=ref.dtype, device=ref.device)
        for i, (g, m) in enumerate(zip(gs, ctx.Ms)):
            if g is None:
                full[i].zero_()
            else:
                full[i, :m].copy_(g)
                if m < ctx.shape[1]:
                    full[i, m:].zero_()
        return (full, *([None] * len(ctx.Ms)))
